// Register-streamed kernels (gate_rs.h, tail_rs.h, cond_rs.h; tools/gate_co.h): the primitives they share and the rules behind
// them.  In these kernels a wave's weights go straight from global memory into a ring of R register stages, the shared operand
// goes into LDS by DMA, and NOTHING but the wave's own counted `s_waitcnt vmcnt(N)` orders either: every vector-memory
// operation is issued from inline asm, where hipcc's wait insertion does not see it, and every N is the number of operations
// the wave issues between the one it waits for and the wait (VmWalk, at the end of this file).
// The rules (each one found the hard way; DESIGN.md "register-streamed kernels: shared rules"):
//   1. MUBUF only (rs_wload).   2. s_nop 4 in front of the VMEM of every statement (rs_wload).   3. LDS-DMA from asm, M0 saved
//   and restored inside the statement (rs_dma16).   4. No branch around a wait that names ring registers (rs_wwait).
//   5. Behind the closing vmcnt(0) every ring stage is named once (rs_touch_all).
#pragma once
#include "gemm_ring.h"
#include <type_traits>

// raw buffer descriptor (stride 0, range check on the byte offset) in SGPRs an asm statement can name: `bytes` bytes from
// byte `skip` of p on (a wave's own window of a stream)
__device__ __forceinline__ u32x4 rs_srd(const void* p, uint32_t bytes, unsigned long long skip = 0) {
    const unsigned long long b = (unsigned long long)(uintptr_t)p + skip;
    return u32x4{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32)) & 0xffffu,
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}

// one 16-byte load per lane, hidden from hipcc's wait bookkeeping; the caller counts vmcnt.
// * A BUFFER load (MUBUF), like the LDS-DMA pieces and the epilogue stores: a counted s_waitcnt vmcnt(N) is only a wait
//   for a particular operation if the operations retire in issue order, and that holds among MUBUF operations.  The first
//   persistent form of the gate loaded the weights with global_load_dwordx4 (the FLAT family, segment global): with
//   out-of-range pieces (which complete at once) and stores between the loads, ~40 % of the overlapped steps came back
//   wrong while every wait had at least its static count of younger operations in program order (FWN_RS_CHECK build):
//   younger MUBUF operations were retiring ahead of older global loads.  (The guide's "flat_*: out of order".)
// * s_nop 4: the descriptor and the offset are scalar arithmetic on kernel arguments, but under SGPR pressure hipcc parks
//   scalars in VGPR lanes and brings them back with v_readlane_b32 right in front of the statement - a VALU write of an
//   SGPR that a VMEM instruction reads needs 5 wait states, and hipcc pads nothing inside an asm (guide section 5.7 item 2):
//   without the pad the gate's NKC = 10 instantiation loaded through garbage bases (memory access faults at random addresses).
template <int OFF>
__device__ __forceinline__ void rs_wload(bf16x8& dst, u32x4 srd, uint32_t soff, uint32_t voff) {
    static_assert(OFF >= 0 && OFF < 4096, "12-bit unsigned immediate");
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(dst) : "v"(voff), "s"(srd), "s"(soff), "i"(OFF) : "memory");
}
// one dword per lane, hidden like rs_wload (the caller counts vmcnt)
__device__ __forceinline__ void rs_dload(float& dst, u32x4 srd, uint32_t voff) {
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, 0 offen" : "=v"(dst) : "v"(voff), "s"(srd) : "memory");
}

// LDS-DMA piece (64 lanes x 16 bytes -> LDS at the wave-uniform byte address lds_addr + lane * 16) issued from inline asm.
// Through the builtin (buf_load16_lds) hipcc knows that LDS writes are in flight and puts an s_waitcnt vmcnt(0) in front of the
// next ds_read / ds_write it emits (it cannot tell that the access is to another slot): in the tail that drained the whole
// prologue - two more o slices and R - 1 weight fragments - in front of the first k-step, and the Wz image in front of phase
// 2 (stamps: 3.6 k cycles at barrier 0).  Issued from asm the pieces are invisible to that pass; every wait for them is a
// counted one.  M0 (the LDS address) is compiler-reserved: saved and restored inside the statement (guide section 5.7).
__device__ __forceinline__ void rs_dma16(u32x4 srd, uint32_t voff, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(srd), "s"(lds_addr) : "memory");
}

// Counted waits: at most N vector-memory operations of the wave still outstanding.  Without an operand (LDS-DMA pieces: nothing
// to name) it is gemm_ring.h's FWN_WAIT_VMCNT; with one or two "+v" operands the registers the awaited loads write are
// redefined AT the wait, so no use of them is scheduled above it.  (Fixed operand counts: an asm operand list takes no pack.)
// ONE statement per wait whatever the run-time case: under `if (first) wait<n0> else wait<n1>` hipcc merges the two arms' "+v"
// operand in a new register and fills it with a v_mov IN FRONT of the s_waitcnt of one arm - a copy of a ring stage whose load
// is still in flight (found in the ISA by tools/check_async_loads.py; it was the persistent gate's race: stale weights in the
// k-steps whose counts differ between the first and the later tiles, whenever the load had not landed by then).  Take the
// smaller count instead: it is safe for both cases (it waits for more).
template <int N>
__device__ __forceinline__ void rs_vmwait() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    FWN_WAIT_VMCNT(N);
}
template <int N, class T>
__device__ __forceinline__ void rs_wwait(T& a) {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory");
}
template <int N, class T>
__device__ __forceinline__ void rs_wwait(T& a, T& b) {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}

// every ring stage made opaque at this point (behind a wait: no use of a stage is scheduled above it); rings [R] and [R][2]
template <int I = 0, int R>
__device__ __forceinline__ void rs_touch_all(bf16x8 (&wq)[R]) {
    if constexpr (I < R) {
        asm volatile("" : "+v"(wq[I]));
        rs_touch_all<I + 1, R>(wq);
    }
}
template <int I = 0, int R>
__device__ __forceinline__ void rs_touch_all(bf16x8 (&wq)[R][2]) {
    if constexpr (I < R) {
        asm volatile("" : "+v"(wq[I][0]), "+v"(wq[I][1]));
        rs_touch_all<I + 1, R>(wq);
    }
}

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): every ring stage and fragment buffer must be a register,
// never an indexed array, so every position of a K loop is a compile-time constant
template <int I, int N, class F>
__device__ __forceinline__ void rs_static_for_impl(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        rs_static_for_impl<I + 1, N>(f);
    }
}
template <int N, class F>
__device__ __forceinline__ void rs_static_for(F&& f) { rs_static_for_impl<0, N>(f); }

// The N of a counted wait: the vector-memory operations a wave issues AFTER a given one (the target) up to the point where it
// waits for it (the query).  A kernel's schedule (RsCount, TrsCount, CrsCount, CoCount) replays the wave's issue order at
// compile time into this recorder - op() per operation, query() per wait, in program order - and reads `result`: -1 = the
// target was not issued in front of the query (nothing to wait for).  Only the first query that matches counts.
struct VmWalk {
    int count = -1, result = -1;
    bool done = false;
    constexpr void op(bool is_target = false) {
        if (count >= 0) ++count;
        if (is_target) count = 0;
    }
    constexpr void query(bool here) {
        if (!done && here) { result = count; done = true; }
    }
};
// three operations and a wait behind operation q for operation t
constexpr int rs_vmwalk_example(int t, int q) {
    VmWalk w;
    for (int i = 0; i < 3; ++i) {
        w.op(i == t);
        w.query(i == q);
    }
    return w.result;
}
static_assert(rs_vmwalk_example(1, 2) == 1, "one operation behind the second at a wait behind the third");
static_assert(rs_vmwalk_example(0, 2) == 2 && rs_vmwalk_example(2, 2) == 0, "the oldest and the youngest");
static_assert(rs_vmwalk_example(1, 0) == -1, "a wait in front of its target has nothing to wait for");
