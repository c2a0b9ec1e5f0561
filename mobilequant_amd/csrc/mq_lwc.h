// The row image and the grid expression of learnable weight clipping, once: included by the fake-quant passes (mq_fake_quant.hip) and by
// the clip search (mq_lwc_search.hip), so that the grid a search scores is the grid the forward later builds.
#pragma once
#include "mq_common.h"

namespace mq {

#pragma clang fp contract(off)

typedef float vf4 __attribute__((ext_vector_type(4)));

template <int VPT>
struct LwcRow {
  vf4 v[VPT];
};

struct LwcGrid {
  float lo, hi, scale, offset, alpha;
};
// sigmoid(bound) * range -> grid: qmodule.py:271-273 then :40-61 (the expression of scale_offset_kernel, mq_fake_quant.hip)
__device__ __forceinline__ LwcGrid lwc_grid(float mn, float mx, float sig_lo, float sig_hi, float qmax, int symmetric) {
  LwcGrid g;
  g.lo = __fmul_rn(sig_lo, mn);
  g.hi = __fmul_rn(sig_hi, mx);
  float beta;
  if (symmetric) {
    g.alpha = (g.lo != g.lo || g.hi != g.hi) ? __fadd_rn(g.lo, g.hi) : fmaxf(fabsf(g.lo), fabsf(g.hi));
    beta = 0.0f;
  } else {
    g.alpha = __fsub_rn(g.hi, g.lo);
    beta = g.lo;
  }
  g.scale = clamp_nan(__fdiv_rn(g.alpha, qmax), 1e-5f, 1e6f);
  g.offset = -rintf(__fdiv_rn(beta, g.scale));
  return g;
}

}  // namespace mq
