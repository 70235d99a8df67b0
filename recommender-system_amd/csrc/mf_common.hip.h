// mf_common.hip.h -- shared constants of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace mf {

constexpr int kWave = 64;

// the 32-bit LDS address of a __shared__ object, and one LDS-DMA transfer of 16 B per lane to the LDS base m0 from inline
// asm (M0 is a reserved register: hipcc re-loads it before each of its own uses; mf_sweep.hip.h says when to wait)
__device__ __forceinline__ unsigned lds_address(const char *p)
{
	return (unsigned) (unsigned long long) (__attribute__((address_space(3))) const char *) p;
}

__device__ __forceinline__ void lds_dma_m0(const char *src, unsigned m0)
{
	asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0) : "memory");
}

}  // namespace mf
