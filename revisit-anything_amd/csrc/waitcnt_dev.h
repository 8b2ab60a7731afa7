// Counted waits of the loops that keep global->LDS DMAs or loads in flight: s_waitcnt takes its count as a literal, so a count that
// comes from a template parameter or from a run-time value is spelled here, once.  vmcnt counts loads AND stores on gfx9 and both
// retire in issue order: "DMA f has landed" = "at most (loads + stores issued after it) outstanding".  Force-inlined, so a kernel's code
// does not depend on which file it is in.
#pragma once
#include <hip/hip_runtime.h>

// s_waitcnt vmcnt(N) for a literal N (the counter has six bits on gfx9)
template <int N>
__device__ __forceinline__ void sv_wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ... and every LDS / scalar-memory operation as well
template <int N>
__device__ __forceinline__ void sv_wait_vm_lgkm0() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(n) for a run-time n: exact for n in 0 .. 22, vmcnt(23) -- stricter than asked -- beyond
__device__ __forceinline__ void sv_wait_vm(int n) {
#define SV_W(v) case v: sv_wait_vm<v>(); break;
  switch (n) {
    SV_W(0) SV_W(1) SV_W(2) SV_W(3) SV_W(4) SV_W(5) SV_W(6) SV_W(7) SV_W(8) SV_W(9) SV_W(10) SV_W(11)
    SV_W(12) SV_W(13) SV_W(14) SV_W(15) SV_W(16) SV_W(17) SV_W(18) SV_W(19) SV_W(20) SV_W(21) SV_W(22)
    default: sv_wait_vm<23>(); break;
  }
#undef SV_W
}

// The wait in front of step p of a queue of QD DMAs in flight, one issued per step: `rem` DMAs were issued after step p's, QD - 1 of
// them while the queue is full, fewer as it drains.  An if-chain over the literal counts (vmcnt(QD - 1) first: the steady state is one
// compare), not the switch above: no jump table in an inner loop.
template <int N>
__device__ __forceinline__ void sv_wait_queue_tail(int rem) {
  if constexpr (N == 0) sv_wait_vm<0>();
  else if (rem == N) sv_wait_vm<N>();
  else sv_wait_queue_tail<N - 1>(rem);
}
template <int QD>
__device__ __forceinline__ void sv_wait_queue(int rem) {
  if (rem >= QD - 1) sv_wait_vm<QD - 1>();
  else sv_wait_queue_tail<QD - 2>(rem);
}
