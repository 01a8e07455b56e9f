// Fragment reads out of LDS that the compiler does not count: shared by gemm_glds_kernel.h and wgrad3x3.hip.
#pragma once
#include "gemm_bf16_common.h"

namespace sat {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- fragment reads of the kernels that transpose an operand out of LDS (ds_read_b64_tr_b16)
// hipcc takes the transpose-read builtin for a possible alias of the LDS-DMA writes still in flight and puts `s_waitcnt vmcnt(0)` in
// front of every group of such reads: each k-step then waits for all the tiles the ring has in flight, the pieces issued a few
// instructions earlier included, and the counted vmcnt waits of the k loop never decide anything.  The ordering that makes a
// fragment read safe is the k loop's own (counted vmcnt, lgkmcnt(0), raw s_barrier ahead of the first read of a stage), so these
// kernels issue their fragment reads as inline asm, which the compiler neither counts nor waits for, and count them by hand:
//   lds_read_*      one LDS read into registers that are NOT valid yet
//   lds_wait<N>     s_waitcnt lgkmcnt(N): every asm read but the newest N has landed (LDS returns in order; N counts the asm reads
//                   issued since - LDS reads and scalar loads the compiler adds in between only make the wait longer, never shorter)
//   frag_landed     names a fragment's registers behind that wait: no consumer (nor the copy that joins the two halves of a
//                   transposed fragment) is scheduled above it
// The row-major operand of a mixed form goes through lds_read_b128 as well, so that one count covers every read of a k-step.
// (tools/check_lds_ring_waits.py holds the generated code to this.)
typedef int i32x2 __attribute__((ext_vector_type(2)));
struct Frag { i32x2 lo, hi; i32x4 q; };      // transposed: k rows 0..3 | 4..7 of the lane's column (lo, hi); row-major: q

__device__ __forceinline__ unsigned lds_addr(const __bf16* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const __bf16*)p;
}
template <int OFF> __device__ __forceinline__ i32x2 lds_read_tr16(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    i32x2 v = {0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
#endif
    return v;
}
template <int OFF> __device__ __forceinline__ i32x4 lds_read_b128(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    i32x4 v = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
#endif
    return v;
}
template <int N> __device__ __forceinline__ void lds_wait() {
    static_assert(N >= 0 && N <= 15, "lgkmcnt field");
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
template <bool TR> __device__ __forceinline__ void frag_landed(Frag& f) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (TR) asm volatile("" : "+v"(f.lo), "+v"(f.hi));
    else asm volatile("" : "+v"(f.q));
#endif
}
template <bool TR> __device__ __forceinline__ bf16x8 frag_value(const Frag& f) {
    if constexpr (TR) return __builtin_bit_cast(bf16x8, __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3));
    else return __builtin_bit_cast(bf16x8, f.q);
}

}  // namespace sat
