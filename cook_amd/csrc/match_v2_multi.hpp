// match_v2_multi.hpp — several pools in one launch: PoolCtx, PoolPack and the _multi / _pack forms of the three kernels of a round.  Part of
// match_v2.hpp: needs eval_block (match_v2_eval.hpp), merge_block (match_v2_merge.hpp) and resolve_round (match_v2_resolve.hpp).
#pragma once

// ---- several pools in one launch ----------------------------------------------------------------------------------------------
// A rank that holds more pools than the GPU runs launch chains at full speed (about four) places them in LOCKSTEP: the
// three launches of a round with blockIdx.z = pool, every pool on its own WinCtl.  Up to MV_PACK pools travel IN the kernel
// arguments (PoolPack: the compiler sees kernel-argument loads — scalar, uniform — where a context record in memory gives it generic
// pointers); more than that read their contexts from a device array.
struct PoolCtx {
  MatchIn in;
  MatchState st;
  V2Buf vb;
};
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_EW) COOK_EVAL_OCCUPANCY match_eval2_multi(const PoolCtx* __restrict__ ctx) {
  __shared__ __attribute__((aligned(16))) char lds[sizeof(EvalLds<GE>)];
  const PoolCtx& c = ctx[blockIdx.z];
  if (blockIdx.x >= c.vb.C) return;
  eval_block<GE>(lds, c.in, c.st, c.vb, c.vb.ctl->head, c.vb.ctl->wcur, blockIdx.x, blockIdx.y, gridDim.y);
}
template <bool GE>
__global__ void __launch_bounds__(COOK_WAVE* MV_MW) match_merge2_multi(const PoolCtx* __restrict__ ctx) {
  const PoolCtx& c = ctx[blockIdx.z];
  merge_block<GE>(c.in, c.vb);
}
template <bool GE>
__global__ void __launch_bounds__(MV_RTHREADS) match_resolve2_multi(const PoolCtx* __restrict__ ctx) {
  __shared__ __attribute__((aligned(16))) char lds[MV_RLDS_BYTES];
  const PoolCtx& c = ctx[blockIdx.z];
  resolve_round<GE>(lds, c.st, c.vb);
}
constexpr int MV_PACK = 4;
template <int N>
struct PoolPack {
  PoolCtx c[N];
};
template <bool GE, int N>
__global__ void __launch_bounds__(COOK_WAVE* MV_EW) COOK_EVAL_OCCUPANCY match_eval2_pack(const PoolPack<N> p) {
  __shared__ __attribute__((aligned(16))) char lds[sizeof(EvalLds<GE>)];
  const PoolCtx& c = p.c[blockIdx.z];
  if (blockIdx.x >= c.vb.C) return;
  eval_block<GE>(lds, c.in, c.st, c.vb, c.vb.ctl->head, c.vb.ctl->wcur, blockIdx.x, blockIdx.y, gridDim.y);
}
template <bool GE, int N>
__global__ void __launch_bounds__(COOK_WAVE* MV_MW) match_merge2_pack(const PoolPack<N> p) {
  const PoolCtx& c = p.c[blockIdx.z];
  merge_block<GE>(c.in, c.vb);
}
template <bool GE, int N>
__global__ void __launch_bounds__(MV_RTHREADS) match_resolve2_pack(const PoolPack<N> p) {
  __shared__ __attribute__((aligned(16))) char lds[MV_RLDS_BYTES];
  const PoolCtx& c = p.c[blockIdx.z];
  resolve_round<GE>(lds, c.st, c.vb);
}
