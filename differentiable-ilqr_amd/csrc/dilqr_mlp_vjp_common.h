// dilqr_mlp_vjp_common.h — what the two weight-gradient units (tu_mlp_vjp.hip,
// tu_mlp2_vjp.hip) share: the wave reduction, the geometry of the slab sum and
// the count of slabs.  The order of summation is part of the units' contract
// (the same bits on every run).
//
// The lane's row load and the body of the slab-sum kernel stay written out in
// each unit: as shared functions (tried both ways: a row struct in
// k_mlp_linearize_vjp, one device function for the slab sum) they compile to
// other instruction streams than the units had (another schedule of the
// one-layer kernel; swapped operands in the sum kernels), and these kernels are
// held to their compiled form.
#pragma once
#include "dilqr_common.h"

namespace dilqr {

constexpr int kVjpDefaultGroups = 512;   // cap on G when the caller gives none
constexpr int kVjpSumSlices = 4;         // slab sum: waves per workgroup, each sums every 4th slab

// the sum over the wave's 64 lanes, in every lane (xor butterfly, a fixed order)
DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

namespace {

// G: one slab per 64-row chunk up to the cap, at least one.  The cap is
// max_waves when the caller gives one, else the default, lowered to slab_cap
// (the slabs a unit's memory budget holds, at least one; by default no budget).
inline long long vjp_groups(long long rows, int max_waves, long long slab_cap = kVjpDefaultGroups) {
  long long cap = slab_cap < 1 ? 1 : slab_cap > kVjpDefaultGroups ? kVjpDefaultGroups : slab_cap;
  if (max_waves > 0) cap = max_waves;
  const long long chunks = (rows + 63) / 64;
  const long long g = chunks < cap ? chunks : cap;
  return g < 1 ? 1 : g;
}

}  // namespace
}  // namespace dilqr
