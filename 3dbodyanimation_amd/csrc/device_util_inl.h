// device_util_inl.h — the small device helpers every kernel unit shares, one definition each (device code only).
#pragma once
#include <hip/hip_runtime.h>

namespace bodyfit {

// 8-byte write-through store (sc1): the payload form of a hand-off to a workgroup on another XCD inside the launch
__device__ __forceinline__ void store_f64_through(double* p, double v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

namespace {

// f64 value of lane `src` (wave-uniform lane id): two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// sum over the 64 lanes of a wave, butterfly: every lane returns the total
__device__ inline double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Block reductions through red[] (one slot per wave of the workgroup), returned to every thread.  The ORDER of the additions
// is part of the contract: the LM solvers compare costs bit for bit between kernels and with the host.
//   block_sum4:  the first four waves' totals as the fixed tree (r0 + r1) + (r2 + r3)   (waves beyond the fourth only store)
//   block_sum_n / block_max_n:  `nwaves` totals folded left to right from 0
// (the butterfly is written out in each: as a call to wave_sum64 the compiler schedules the staging store differently, and
//  the kernels' code is kept instruction for instruction)
__device__ inline double block_sum4(double v, double* red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ inline double block_sum_n(double v, double* red, int tid, int nwaves) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nwaves; ++w) s += red[w];
  return s;
}
__device__ inline double block_max_n(double v, double* red, int tid, int nwaves) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nwaves; ++w) s = fmax(s, red[w]);
  return s;
}

// Huber's rho(s) of a squared norm s and its derivative (Ceres HuberLoss; delta <= 0: no loss)
__device__ inline double huber_rho(double delta, double s, double* rho1) {
  const double b = delta * delta;
  if (delta > 0.0 && s > b) {
    const double rt = sqrt(s);
    *rho1 = delta / rt;
    return 2.0 * delta * rt - b;
  }
  *rho1 = 1.0;
  return s;
}

// The temporal term (Vec3DiffCost, include/MultiFrameBA.h:121-142) orders its rows rootT, rootAA, then the joints:
// temporal_row(s): the row that constrains frame parameter s >= 1 (the scale, s = 0, has none); priors_inl.h temporal_rows
// writes the rows with the inverse map
__device__ __forceinline__ int temporal_row(int s) { return (s >= 7) ? (s - 7 + 6) : (s >= 4 ? (s - 4) : (s - 1 + 3)); }

}  // namespace
}  // namespace bodyfit
