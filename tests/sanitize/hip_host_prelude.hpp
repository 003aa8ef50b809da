// Force-included in front of lazy_bucket_main.cpp (lazy_bucket.mk) and pairing_pieces_main.cpp (pairing_pieces.mk): what the device
// headers under csrc/ need beyond ROCm's own headers to compile as plain C++ for the CPU.  Outside HIP mode <hip/hip_runtime.h> defines
// __device__, __global__ and friends as empty; the builtins of the kernel BODIES get single-lane stand-ins here so that the headers parse and
// link.  The host programs call no kernel, only the __device__ functions of lazy29.hpp, msm_kernels.hpp and pairing.hpp, so none of these is
// ever executed.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#ifndef __launch_bounds__
#define __launch_bounds__(...)
#endif
using std::max;
using std::min;
// (defined, not only declared: the few kernels that are not templates are compiled, though never called)
inline const dim3 threadIdx{}, blockIdx{}, blockDim{}, gridDim{};
inline void __syncthreads() {}
template <class T> T atomicAdd(T* p, T v) { const T o = *p; *p = o + v; return o; }
template <class T> T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
template <class T> T atomicMax(T* p, T v) { const T o = *p; if (o < v) *p = v; return o; }
template <class T> T atomicOr(T* p, T v) { const T o = *p; *p = o | v; return o; }
template <class T> T atomicExch(T* p, T v) { const T o = *p; *p = v; return o; }
template <class T> T atomicCAS(T* p, T c, T v) { const T o = *p; if (o == c) *p = v; return o; }
template <class T> T __shfl(T v, int, int = 64) { return v; }
template <class T> T __shfl_up(T v, unsigned, int = 64) { return v; }
template <class T> T __shfl_down(T v, unsigned, int = 64) { return v; }
template <class T> T __shfl_xor(T v, int, int = 64) { return v; }
// the dynamic LDS arrays of those kernels: `extern __shared__` is a plain `extern` here, so they need a definition to link
namespace cg { inline uint32_t lds_cnt[1], lds_u32[1]; }
