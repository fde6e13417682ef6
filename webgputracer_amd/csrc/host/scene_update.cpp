// scene_update.cpp — Scene::UpdateTriangles: the C++ mirror of wgt_update_triangles (no reference
// counterpart: the reference's scenes do not move).  In a translation unit of its own, so that
// programs that link scene.cpp without the device runtime need only the upload's symbol.
#include <iostream>

#include "../../../include/wgt/scene.h"

namespace wgt {

bool Scene::UpdateTriangles(wgt_ctx* ctx) {
  if (!uploaded_ || ctx != ctx_) {
    std::cerr << "[WebGPUTracer] triangle update failed: the scene is not uploaded to this context" << std::endl;
    return false;
  }
  if (tris_.size() != uploaded_tris_) {
    std::cerr << "[WebGPUTracer] triangle update failed: " << tris_.size() << " triangles, " << uploaded_tris_
              << " uploaded (InitBuffers adds or removes triangles)" << std::endl;
    return false;
  }
  auto t = PackTriangles();
  int rc = wgt_update_triangles(ctx, t.empty() ? nullptr : t.data(), (uint32_t)t.size());
  if (rc != WGT_OK) {
    std::cerr << "[WebGPUTracer] triangle update failed: " << wgt_last_error(ctx) << std::endl;
    return false;
  }
  return true;
}

// The mirror of wgt_rebuild_triangles: the count may have changed since InitBuffers.
bool Scene::RebuildTriangles(wgt_ctx* ctx) {
  if (!uploaded_ || ctx != ctx_) {
    std::cerr << "[WebGPUTracer] triangle rebuild failed: the scene is not uploaded to this context" << std::endl;
    return false;
  }
  auto t = PackTriangles();
  int rc = wgt_rebuild_triangles(ctx, t.empty() ? nullptr : t.data(), (uint32_t)t.size());
  if (rc != WGT_OK) {
    std::cerr << "[WebGPUTracer] triangle rebuild failed: " << wgt_last_error(ctx) << std::endl;
    return false;
  }
  uploaded_tris_ = t.size();
  return true;
}

}  // namespace wgt
