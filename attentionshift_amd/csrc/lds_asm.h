// Shared LDS, LDS-DMA and compile-time-loop helpers of the kernels (device only, gfx950 / CDNA4).
//
// Why the reads are hidden.  After an LDS-DMA (global_load_lds_*: global memory -> LDS with no staging VGPRs, counted on
// vmcnt) hipcc drains vmcnt(0) before any LDS read it can see: it cannot prove that the read does not alias the DMA
// destination.  In a ring of tiles that drain would wait for the tiles still in flight and collapse the ring to depth 0.
// So the fragment reads of such kernels are issued in inline asm (lds_read*), where the compiler sees neither an LDS access
// nor a counter, and they are completed by lds_wait<LEFT>(...).
//
// What the wait must name.  lds_wait is ONE asm statement, `s_waitcnt lgkmcnt(LEFT)`, that lists EVERY destination register
// of the reads it completes as read-write ("+v"): that makes the statement a definition of those registers, so no use of
// them can be moved above it and nothing is consumed early (cdna_hip_programming.md section 5.7, form ii).  LDS returns in
// order, so LEFT = the number of later reads that may stay in flight.  A sched_barrier(0) follows (rule 18): the MFMAs
// behind the wait must not be hoisted over it either.  One statement per wait is what the kernels were tuned with.
//
// The LDS-DMA.  lds_dma16 / lds_dma4 use the saddr form: 64 lanes x 16 (4) bytes from sbase + voff[lane] go to LDS
// [m0 + 16 (4) * lane].  m0 is saved and restored inside the same statement, so the compiler's own uses of m0 never see the
// change (cdna_hip_programming.md 5.7); `sbase` and `lds_dst` must be wave-uniform.  A kernel that issues its DMA this way
// and never through a builtin shows hipcc no vm-counted LDS write at all, and may then read LDS in plain C++.
//
// A second kernel file that needs one of these includes this header; it does not copy it.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;    // plain vector types: staging arrays stay in VGPRs
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const char* lds_ptr;  // 32-bit LDS pointer: lane pointer + constant folds into the DS immediate

#ifdef __HIPCC__
// shared-memory address as the 32-bit value the DS and LDS-DMA instructions take
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}

__device__ __forceinline__ void lds_dma16(unsigned voff, const char* sbase, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void lds_dma4(unsigned voff, const char* sbase, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// hidden reads.  Immediate-offset forms: the per-lane address register is loop-invariant, ring slot / row block are
// immediates.  The immediate is 16 bits: the part of OFF above it becomes one v_add (for OFF < 65536 it folds away).
__device__ __forceinline__ void lds_read128(u32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr));
}
template <int OFF> __device__ __forceinline__ void lds_read128_i(u32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr + (unsigned)(OFF & ~0xFFFF)), "n"(OFF & 0xFFFF));
}
// transposing read: every 16-lane group reads a 4-row x 16-column bf16 block, lane c receives column c's four rows
template <int OFF> __device__ __forceinline__ void lds_read_tr64_i(u32x2& dst, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr + (unsigned)(OFF & ~0xFFFF)), "n"(OFF & 0xFFFF));
}

// the wait that completes hidden reads, at the arities the kernels use (T: u32x4 or u32x2)
template <int LEFT, typename T> __device__ __forceinline__ void lds_wait(T& a, T& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(LEFT));
  __builtin_amdgcn_sched_barrier(0);
}
template <int LEFT, typename T> __device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(LEFT));
  __builtin_amdgcn_sched_barrier(0);
}
template <int LEFT, typename T> __device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d, T& e, T& f) {
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "n"(LEFT));
  __builtin_amdgcn_sched_barrier(0);
}
template <int LEFT, typename T> __device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d, T& e, T& f, T& g, T& h) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(LEFT));
  __builtin_amdgcn_sched_barrier(0);
}
template <int LEFT, typename T>
__device__ __forceinline__ void lds_wait(T& a, T& b, T& c, T& d, T& e, T& f, T& g, T& h, T& i, T& j, T& k, T& l) {
  asm volatile("s_waitcnt lgkmcnt(%12)"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j), "+v"(k), "+v"(l)
               : "n"(LEFT));
  __builtin_amdgcn_sched_barrier(0);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression
// (ring slots as immediates)
template <int... I, typename F> __device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// bf16 fragment from two transposing reads through the compiler's builtin (hipcc tracks their lgkmcnt): lane (li, half)
// gets rows [8 half .. 8 half + 7] of column li of a 16-row x 32-column block (p0: rows +0..3, p1: rows +4..7)
__device__ __forceinline__ void lds_frag_tr(Frag<__bf16>& f, lds_ptr p0, lds_ptr p1) {
  const i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p0);
  const i16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p1);
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  const i16x8 w = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  f.v = __builtin_bit_cast(bf16x8, w);
}

// Swizzles of the 16-byte chunk index inside a tile row (chunk c of row r is kept at position c ^ swz(r), applied on the
// DMA's source address), so that LDS reads meet no bank conflict.
// lds_swz_row<KS>: for ds_read_b128 row fragments.  Each lane group the read is serviced in (16 lanes: rows {0-3, 12-15,
// 20-27} or {4-11, 16-19, 28-31} of a 32-row block, one chunk column) covers the 16 slots of a 256-byte bank row once.
// KS = 2, 64-byte rows (4 chunks): (row >> 2) & 3.  KS = 4, 128-byte rows (8 chunks): ((row >> 1) & 3) | ((row >> 4) & 1) << 2.
template <int KS> __device__ __forceinline__ int lds_swz_row(int r) {
  return KS == 2 ? ((r >> 2) & 3) : (((r >> 1) & 3) | (((r >> 4) & 1) << 2));
}
// lds_swz_tr: 128-byte rows read both ways.  The ds_read_b128 row fragments: the eight rows of one parity get eight distinct
// positions.  The transposing reads (a 32-lane group covers 4 rows x 4 chunks): rows r, r + 2 land in different halves of
// the 128-byte line.
__device__ __forceinline__ int lds_swz_tr(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
#endif
