// stage_check.h — what every staging layout of the synchronous image passes (launch_plan.h StageLayout)
// must satisfy, for the plan fuzzers: each states its call's parts (bytes, upload source, fetch
// destination) in order, from the API's plane sizes alone, and check_stage compares.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../webgputracer_amd/csrc/host/launch_plan.h"

// A distinct non-null address per buffer (never dereferenced), so that a part wired to the wrong
// buffer shows.
inline void* fake_ptr(int i) { return (void*)(uintptr_t)(0x10000u * (unsigned)(i + 1)); }

struct StageWant {
  uint64_t bytes;   // 0: the part is absent
  const void* src;  // uploaded from, or null
  void* dst;        // fetched to, or null
};

// Returns the number of failed checks (each printed with the part it concerns).
inline int check_stage(const char* name, const wgt::StageLayout& l, const StageWant* want, int n_want) {
  int bad = 0;
  const auto fail = [&](const char* what, int k) {
    std::fprintf(stderr, "%s: part %d: %s\n", name, k, what);
    ++bad;
  };
  if (l.n != n_want || l.n > wgt::StageLayout::kMaxParts) {
    fail("part count", l.n);
    return bad;
  }
  char* const base = (char*)(uintptr_t)0x7000000;  // 256-B aligned; arithmetic only
  unsigned __int128 sum = 0;  // of the aligned sizes, where no size_t can wrap
  if (l.off[0] != 0) fail("the first offset is not 0", 0);
  for (int k = 0; k < l.n; ++k) {
    const wgt::StagePart& p = l.part[k];
    if (p.bytes != want[k].bytes) fail("byte count", k);
    if (p.src != (want[k].bytes ? want[k].src : nullptr)) fail("upload source", k);
    if (p.dst != (want[k].bytes ? want[k].dst : nullptr)) fail("fetch destination", k);
    if (l.off[k] % 256 != 0) fail("offset not 256-B aligned", k);
    if ((unsigned __int128)l.off[k] != sum) fail("offset is not the sum of the aligned parts before it", k);
    sum += ((unsigned __int128)want[k].bytes + 255) / 256 * 256;
    if (l.off[k + 1] < l.off[k] || l.off[k + 1] - l.off[k] < p.bytes) fail("overlaps the next part", k);
    void* const at = l.at(base, k);
    if (p.bytes == 0 ? at != nullptr : at != base + l.off[k]) fail("accessor", k);
  }
  if ((unsigned __int128)l.bytes() != sum || l.bytes() % 256 != 0) fail("total", l.n);
  return bad;
}
