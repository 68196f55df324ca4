// lstm_point.h -- the element-wise LSTM step of one (row, unit): the one definition every LSTM schedule calls.
//
// The kernels differ in where the operands come from (registers, LDS, global), in their masks and in how results leave;
// the arithmetic between is this file's, so two schedules that are handed the same f32 operands produce the same bits.
// Every rounding below is written out (explicit fma, contraction off): left to -ffp-contract the optimizer fused
// `1 - tc*tc`, `1 - g*g` and the carry add at some call sites and instantiations and not at others.
//
// Forward, from the four pre-activations p_i, p_f, p_g, p_o (gate order i, f, g, o) and c_prev; fl() is one f32 rounding:
//   i = sigmoidf_(p_i), f = sigmoidf_(p_f), g = tanhf_(p_g), o = sigmoidf_(p_o)
//   c = fma(f, c_prev, fl(i*g))                    h = fl(o * tanhf_(c))
//
// Backward, from dh (all of its terms already summed), the gates, c (this step's), c_prev and the incoming carry dc_in
// (dL/dc of the step after, times that step's f; there is none at the last step):
//   tc = tanhf_(c)                                 b  = fma(-tc, tc, 1)
//   x  = fl(dh*o)                                  dc = carry ? fma(x, b, dc_in) : fl(x*b)
//   dp_i = fl(fl(fl(dc*g)*i) * fl(1-i))            dp_f = fl(fl(fl(dc*c_prev)*f) * fl(1-f))
//   dp_g = fl(fl(dc*i) * fma(-g, g, 1))            dp_o = fl(fl(fl(dh*tc)*o) * fl(1-o))
//   dc_out = fl(dc*f)                              (the carry handed to the step before)
#pragma once
#include "common.h"

// Gate nonlinearities on the hardware transcendental units (v_exp_f32 / v_rcp_f32, ~1 ulp each): the libm
// expf/tanhf expand to ~30-40 instructions with branches and made the cell epilogue cost more than its GEMM.
// Absolute error ~1e-7 on values in (-1,1): inside the 1e-4 parity budget (checked by the LSTM parity tests).
// (__builtin_amdgcn_rcpf = one v_rcp_f32, 1 ulp; __frcp_rn expands to the ten-instruction correctly-rounded division)
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
  // tanh(x) = 1 - 2/(1+exp(2x)); exp overflow -> rcp(inf) = 0 -> 1, underflow -> 1-2 = -1
  // (an explicit fma: left to -ffp-contract the compiler fused this differently in different unrolled copies of an
  //  epilogue, and a row's result then depended on which tile slot of a wave it occupied)
  return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)), 1.0f);
}

struct LstmPointFwd {
  float ig, fg, gg, og, c, h;
};
__device__ __forceinline__ LstmPointFwd lstm_point_fwd(float p_i, float p_f, float p_g, float p_o, float c_prev) {
  LstmPointFwd r;
  r.ig = sigmoidf_(p_i), r.fg = sigmoidf_(p_f), r.gg = tanhf_(p_g), r.og = sigmoidf_(p_o);
  r.c = __builtin_fmaf(r.fg, c_prev, r.ig * r.gg);
  r.h = r.og * tanhf_(r.c);
  return r;
}

struct LstmPointBwd {
  float dp[4];  // d(loss)/d(pre-activation), gate order i, f, g, o
  float dc;     // the outgoing carry
};
// carry: whether a step after this one exists; dc_in is not used without one (it may be any value)
__device__ __forceinline__ LstmPointBwd lstm_point_bwd(float dh, float ig, float fg, float gg, float og, float c, float c_prev,
                                                       bool carry, float dc_in) {
#pragma clang fp contract(off)
  LstmPointBwd r;
  const float tc = tanhf_(c);
  const float b = __builtin_fmaf(-tc, tc, 1.f);
  const float x = dh * og;
  const float dc = carry ? __builtin_fmaf(x, b, dc_in) : x * b;
  const float d_o = dh * tc;
  const float d_i = dc * gg, d_f = dc * c_prev, d_g = dc * ig;
  r.dc = dc * fg;
  r.dp[0] = d_i * ig * (1.f - ig);
  r.dp[1] = d_f * fg * (1.f - fg);
  r.dp[2] = d_g * __builtin_fmaf(-gg, gg, 1.f);
  r.dp[3] = d_o * og * (1.f - og);
  return r;
}
