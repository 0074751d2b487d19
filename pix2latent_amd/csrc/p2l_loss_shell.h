// Host-side shell of the projection loss (weighted L1 + beta * weighted LPIPS) shared by the VGG16, AlexNet and
// SqueezeNet plans (p2l_plan.hip, p2l_plan_alex.hip, p2l_plan_squeeze.hip), plus the two helpers every plan file
// uses (Arena, RET_IF).  Library-internal: everything has internal linkage, nothing is exported.
// A plan supplies its activation layout (a struct derived from LossLayout whose taps it fills), its feature
// forward (a callable) and the walk back through its backbone; the argument checks, the L1 term, the per-tap
// LPIPS launches and the reductions are here, once.  No allocation, no synchronisation, no device read: the
// entry points run under graph capture.
#pragma once
#include "p2l_common.h"

namespace {

struct Arena {
  size_t off = 0;  // in floats
  size_t take(size_t n) {
    const size_t o = off;
    off += (n + 63) & ~(size_t)63;
    return o;
  }
};

#define RET_IF(x)          \
  do {                     \
    int _rc = (x);         \
    if (_rc) return _rc;   \
  } while (0)

// descriptor of a square-kernel p2l_gconv_fwd launch on dense NHWC tensors
inline P2LGConv gconv_desc(int B, int Hi, int Wi, int Cin, int Cout, int K, int S, int P) {
  P2LGConv d{};
  d.B = B; d.Hi = Hi; d.Wi = Wi; d.Cin = Cin; d.Cout = Cout; d.KH = K; d.KW = K; d.stride = S;
  d.pad = P; d.x_ld = Cin; d.y_ld = Cout; d.res_ld = Cout; d.mask_ld = Cout;
  return d;
}

// The LPIPS taps of one network at one image size: filled by the plan's layout, then bound to the caller's
// descriptor (lin) and P2LLossCache / P2LLossCache7 (by pointer: nothing of the caller's is read before the checks)
struct LossTaps {
  int n = 0;                         // <= 7
  int h[7], w[7], C[7];
  size_t y[7];                       // workspace offset (floats) of the tap's post-ReLU activation
  const float* const* lin = nullptr;
  float* const* nft = nullptr;
  float* const* wt = nullptr;
  float* const* wsum = nullptr;
  int P(int k) const { return h[k] * w[k]; }
  template <class Net, class Cache>
  void bind(const Net* v, const Cache* c) {
    if (v) lin = v->lin;
    if (c) { nft = c->nft; wt = c->wt; wsum = &c->wsum; }
  }
};

// what every plan's arena holds behind its activations, in this order (plan-specific regions follow it)
struct LossTail {
  size_t tgt16;        // prepare: target in NHWC16
  size_t wsrc;         // prepare: per-pixel weight map
  size_t part;         // loss partial sums (L1 or the largest tap)
  size_t lp, l1;       // per-sample partial losses
  size_t gs;           // per-sample gradient scale
  size_t ga, gb, gtap; // backward scratch
  void take(Arena& a, int B, int H, int W, const LossTaps& T, size_t max_act) {
    tgt16 = a.take((size_t)B * H * W * 16);
    wsrc = a.take((size_t)B * H * W);
    size_t maxpart = (size_t)p2l_l1_loss_nblk(H, W);
    for (int k = 0; k < T.n; ++k) {
      const size_t nb = (size_t)p2l_lpips_tap_nblk(T.P(k), T.C[k]);
      if (nb > maxpart) maxpart = nb;
    }
    part = a.take((size_t)B * maxpart);
    lp = a.take(B);
    l1 = a.take(B);
    gs = a.take(B);
    ga = a.take(max_act);
    gb = a.take(max_act);
    gtap = a.take(max_act);
  }
};

struct LossLayout {                  // base of AxLayout / SqLayout / PLLayout
  LossTaps taps;
  LossTail tail;
  size_t total;
};

inline size_t loss_cache_floats(const LossTaps& T, int B, size_t* nft_off, size_t* wt_off, size_t* wsum_off) {
  Arena a;
  for (int k = 0; k < T.n; ++k) {
    nft_off[k] = a.take((size_t)B * T.P(k) * T.C[k]);
    wt_off[k] = a.take((size_t)B * T.P(k));
  }
  *wsum_off = a.take(B);
  return a.off;
}

inline bool loss_ws_ok(const LossLayout& L, const void* ws, size_t ws_bytes) {
  return ws && ws_bytes >= L.total * sizeof(float) && L.taps.nft;
}

// features(img16): the plan's feature forward into the workspace
template <class F>
int loss_prepare(const LossLayout& L, const float* target, const float* weight, const float* loss_mask, int B,
                 int H, int W, void* ws, size_t ws_bytes, void* st, F&& features) {
  const LossTaps& T = L.taps;
  if (!loss_ws_ok(L, ws, ws_bytes) || !target) return P2L_EWS;
  float* Wk = (float*)ws;
  if (weight) {
    RET_IF(p2l_weight_sum(weight, loss_mask, *T.wsum, B, 3 * H * W, st));
    RET_IF(p2l_weight_map(weight, loss_mask, Wk + L.tail.wsrc, B, H, W, st));
    for (int k = 0; k < T.n; ++k)
      RET_IF(p2l_bilinear_adjoint(Wk + L.tail.wsrc, T.wt[k], B, H, W, T.h[k], T.w[k], st));
  }
  if (T.lin) {
    RET_IF(p2l_nchw3_to_nhwc16(target, Wk + L.tail.tgt16, B, H, W, st));
    RET_IF(features(Wk + L.tail.tgt16));
    for (int k = 0; k < T.n; ++k)
      RET_IF(p2l_lpips_normalize(Wk + T.y[k], T.nft[k], (int64_t)B * T.P(k), T.C[k], st));
  }
  return P2L_OK;
}

template <class F>
int loss_fwd(const LossLayout& L, const float* img16, const float* target, const float* weight,
             const float* loss_mask, float beta, int use_lpips, int B, int H, int W, void* ws, size_t ws_bytes,
             float* loss, float* loss_l1, float* loss_lpips, void* st, F&& features) {
  const LossTaps& T = L.taps;
  if (!loss_ws_ok(L, ws, ws_bytes) || !img16 || !loss) return P2L_EWS;
  float* Wk = (float*)ws;
  float* l1 = loss_l1 ? loss_l1 : Wk + L.tail.l1;
  float* lp = loss_lpips ? loss_lpips : Wk + L.tail.lp;
  RET_IF(p2l_l1_loss_fwd(img16, target, weight, loss_mask, *T.wsum, l1, Wk + L.tail.part, B, H, W, st));
  RET_IF(p2l_vec_scale_div(l1, nullptr, loss, B, 1.f, st));
  if (use_lpips) {
    if (!T.lin) return P2L_EINVAL;
    RET_IF(features(img16));
    for (int k = 0; k < T.n; ++k) {
      const int P = T.P(k), C = T.C[k];
      RET_IF(p2l_lpips_tap_fwd(Wk + T.y[k], T.nft[k], (int64_t)P * C, T.lin[k], T.wt[k], P, Wk + L.tail.part, B,
                               P, C, st));
      RET_IF(p2l_reduce_rows(Wk + L.tail.part, lp, B, p2l_lpips_tap_nblk(P, C), 1.f, *T.wsum, k > 0, st));
    }
    RET_IF(p2l_reduce_rows(lp, loss, B, 1, beta, nullptr, 1, st));
  }
  return P2L_OK;
}

// One backward call between loss_bwd_begin and loss_bwd_end: its arguments, the three scratch buffers and the
// tap gradient.  The plan walks its backbone from the last tap down to dimg16 in between.
struct LossBwd {
  const LossLayout* L;
  const float *img16, *target, *weight, *loss_mask, *gloss;
  int use_lpips, B, H, W;
  float *Wk, *dimg16;
  void* st;
  bool done = false;                 // L1 only: loss_bwd_begin wrote dimg16, nothing is left to do
  float *ga, *gb, *gtap;             // ga: gradient w.r.t. the PRE-ReLU output of the current layer (masked)
  // gtap = d (beta * LPIPS) / d (tap k's activation)
  int tap(int k) const {
    const LossTaps& T = L->taps;
    const int P = T.P(k), C = T.C[k];
    return p2l_lpips_tap_bwd(Wk + T.y[k], T.nft[k], (int64_t)P * C, T.lin[k], T.wt[k], P, Wk + L->tail.gs, gtap,
                             B, P, C, st);
  }
};

inline int loss_bwd_begin(const LossLayout& L, const float* img16, const float* target, const float* weight,
                          const float* loss_mask, float beta, int use_lpips, const float* gloss, int B, int H,
                          int W, void* ws, size_t ws_bytes, float* dimg16, void* st, LossBwd& bw) {
  const LossTaps& T = L.taps;
  if (!loss_ws_ok(L, ws, ws_bytes) || !img16 || !gloss || !dimg16) return P2L_EWS;
  float* Wk = (float*)ws;
  bw = LossBwd{&L, img16, target, weight, loss_mask, gloss, use_lpips, B, H, W, Wk, dimg16, st, !use_lpips,
               Wk + L.tail.ga, Wk + L.tail.gb, Wk + L.tail.gtap};
  if (!use_lpips)
    return p2l_l1_loss_bwd(img16, target, weight, loss_mask, *T.wsum, gloss, dimg16, B, H, W, 0, st);
  if (!T.lin) return P2L_EINVAL;
  // gs[b] = gloss[b] * beta / wsum[b]
  return p2l_vec_scale_div(gloss, *T.wsum, Wk + L.tail.gs, B, beta, st);
}

// behind the launch that wrote d (beta * LPIPS) / d img16 into dimg16
inline int loss_bwd_end(const LossBwd& bw) {
  if (bw.use_lpips == 2) return P2L_OK;   // PerceptualLoss on its own: no L1 term
  return p2l_l1_loss_bwd(bw.img16, bw.target, bw.weight, bw.loss_mask, *bw.L->taps.wsum, bw.gloss, bw.dimg16,
                         bw.B, bw.H, bw.W, 1, bw.st);
}

}  // namespace
