// The constants of the arena, tile and chain layout that host-only code needs as well as the kernels: plain C++, no HIP.
// Included by kernel_common.h (the kernels) and stream_plan.h (the push planner, which also compiles without hipcc).
#pragma once

namespace {

constexpr int TILE = 64;       // frames per tile (= lanes of the per-frame phase)
constexpr int WG = 512;        // threads per workgroup (8 waves)
constexpr int NWAVE = WG / 64;
constexpr int PCM_ALIGN = 8;   // utterance starts are multiples of this many samples
constexpr int PCM_HEAD = 8;    // samples of padding before the first utterance (x[-2..-1] of frame 0 is loaded)
constexpr int PCM_TAIL = 512;  // padding after the last one: the generic instantiation loads 16 rows of 32 samples whatever the window

}  // namespace
