// ProjectionLoss with the LPIPS-AlexNet network (the reference default,
// pix2latent/loss_functions.py:86-100 `ProjectionLoss(lpips_net='alex', beta=10)`,
// :126-148 PerceptualLoss -> lpips.LPIPS(net='alex', spatial=True)).  Same structure as
// the VGG16 plan in p2l_plan.hip: target features / adjoint-resized weight maps cached per
// target, weighted spatial sum evaluated at tap resolution, dgrad-only backward.
#include "p2l_loss_shell.h"

namespace {

const int kCin[5] = {16, 64, 192, 384, 256};
const int kCout[5] = {64, 192, 384, 256, 256};
const int kK[5] = {11, 5, 3, 3, 3};
const int kS[5] = {4, 1, 1, 1, 1};
const int kP[5] = {2, 2, 1, 1, 1};

struct AxLayout : LossLayout {
  int h[5], w[5];          // output grid of conv i (= tap i)
  int hp[2], wp[2];        // pooled grids (input of conv 1 and conv 2)
  size_t y[5], p[2];
};

int ax_layout(int B, int H, int W, AxLayout& L) {
  if (B < 1 || H < 35 || W < 35) return P2L_EINVAL;     // two 3/2 pools behind an 11/4 conv
  L.h[0] = (H + 4 - 11) / 4 + 1; L.w[0] = (W + 4 - 11) / 4 + 1;
  L.hp[0] = (L.h[0] - 3) / 2 + 1; L.wp[0] = (L.w[0] - 3) / 2 + 1;
  L.h[1] = L.hp[0]; L.w[1] = L.wp[0];
  L.hp[1] = (L.h[1] - 3) / 2 + 1; L.wp[1] = (L.w[1] - 3) / 2 + 1;
  for (int i = 2; i < 5; ++i) { L.h[i] = L.hp[1]; L.w[i] = L.wp[1]; }
  if (L.hp[1] < 1 || L.wp[1] < 1) return P2L_EINVAL;
  Arena a;
  size_t max_act = 0;
  for (int i = 0; i < 5; ++i) {
    const size_t n = (size_t)B * L.h[i] * L.w[i] * kCout[i];
    L.y[i] = a.take(n);
    if (n > max_act) max_act = n;
  }
  L.p[0] = a.take((size_t)B * L.hp[0] * L.wp[0] * kCout[0]);
  L.p[1] = a.take((size_t)B * L.hp[1] * L.wp[1] * kCout[1]);
  L.taps.n = 5;
  for (int k = 0; k < 5; ++k) { L.taps.h[k] = L.h[k]; L.taps.w[k] = L.w[k]; L.taps.C[k] = kCout[k]; L.taps.y[k] = L.y[k]; }
  L.tail.take(a, B, H, W, L.taps, max_act);
  L.total = a.off;
  return P2L_OK;
}

// AlexNet features on an NHWC16 image: y[i] = relu(conv_i), p[j] = pooled inputs
int alex_forward(const P2LAlexLpips* v, const float* img16, int B, int H, int W, float* Wk,
                 const AxLayout& L, void* st) {
  {
    P2LGConv d = gconv_desc(B, H, W, 16, 64, 11, 4, 2);
    d.relu = 1;
    RET_IF(p2l_gconv_fwd(&d, img16, v->w[0], v->b[0], v->in_s, v->in_t, nullptr, nullptr,
                         Wk + L.y[0], st));
  }
  RET_IF(p2l_maxpool3s2_fwd(Wk + L.y[0], Wk + L.p[0], B, L.h[0], L.w[0], 64, st));
  {
    P2LGConv d = gconv_desc(B, L.hp[0], L.wp[0], 64, 192, 5, 1, 2);
    d.relu = 1;
    RET_IF(p2l_gconv_fwd(&d, Wk + L.p[0], v->w[1], v->b[1], nullptr, nullptr, nullptr, nullptr,
                         Wk + L.y[1], st));
  }
  RET_IF(p2l_maxpool3s2_fwd(Wk + L.y[1], Wk + L.p[1], B, L.h[1], L.w[1], 192, st));
  const float* x = Wk + L.p[1];
  for (int i = 2; i < 5; ++i) {
    P2LGConv d = gconv_desc(B, L.h[i], L.w[i], kCin[i], kCout[i], 3, 1, 1);
    d.relu = 1;
    RET_IF(p2l_gconv_fwd(&d, x, v->w[i], v->b[i], nullptr, nullptr, nullptr, nullptr,
                         Wk + L.y[i], st));
    x = Wk + L.y[i];
  }
  return P2L_OK;
}

}  // namespace

extern "C" size_t p2l_alex_cache_floats(int B, int H, int W, size_t nft_off[5], size_t wt_off[5],
                                        size_t* wsum_off) {
  AxLayout L;
  if (ax_layout(B, H, W, L)) return 0;
  return loss_cache_floats(L.taps, B, nft_off, wt_off, wsum_off);
}

extern "C" size_t p2l_alexloss_ws_bytes(int B, int H, int W) {
  AxLayout L;
  if (ax_layout(B, H, W, L)) return 0;
  return L.total * sizeof(float);
}

extern "C" int p2l_alexloss_prepare(const P2LAlexLpips* v, const float* target,
                                    const float* weight, const float* loss_mask, int B, int H,
                                    int W, const P2LLossCache* cache, void* ws, size_t ws_bytes,
                                    void* st) {
  AxLayout L;
  RET_IF(ax_layout(B, H, W, L));
  L.taps.bind(v, cache);
  return loss_prepare(L, target, weight, loss_mask, B, H, W, ws, ws_bytes, st, [&](const float* img16) {
    return alex_forward(v, img16, B, H, W, (float*)ws, L, st);
  });
}

extern "C" int p2l_alexloss_fwd(const P2LAlexLpips* v, const float* img16, const float* target,
                                const float* weight, const float* loss_mask,
                                const P2LLossCache* cache, float beta, int use_lpips, int B,
                                int H, int W, void* ws, size_t ws_bytes, float* loss,
                                float* loss_l1, float* loss_lpips, void* st) {
  AxLayout L;
  RET_IF(ax_layout(B, H, W, L));
  L.taps.bind(v, cache);
  return loss_fwd(L, img16, target, weight, loss_mask, beta, use_lpips, B, H, W, ws, ws_bytes, loss, loss_l1,
                  loss_lpips, st, [&](const float* x) { return alex_forward(v, x, B, H, W, (float*)ws, L, st); });
}

extern "C" int p2l_alexloss_bwd(const P2LAlexLpips* v, const float* img16, const float* target,
                                const float* weight, const float* loss_mask,
                                const P2LLossCache* cache, float beta, int use_lpips,
                                const float* gloss, int B, int H, int W, void* ws,
                                size_t ws_bytes, float* dimg16, void* st) {
  AxLayout L;
  RET_IF(ax_layout(B, H, W, L));
  L.taps.bind(v, cache);
  LossBwd bw;
  RET_IF(loss_bwd_begin(L, img16, target, weight, loss_mask, beta, use_lpips, gloss, B, H, W, ws, ws_bytes, dimg16,
                        st, bw));
  if (bw.done) return P2L_OK;
  float* Wk = (float*)ws;
  float *ga = bw.ga, *gb = bw.gb, *gtap = bw.gtap;
  // relu5 is only consumed by its tap
  RET_IF(bw.tap(4));
  RET_IF(p2l_relu_mask(Wk + L.y[4], 256, gtap, 256, ga, 256, (int64_t)B * L.h[4] * L.w[4], 256, st));
  // conv4, conv3 (3x3 chain): dgrad conv + tap gradient as residual + ReLU mask of the input
  for (int i = 4; i >= 3; --i) {
    RET_IF(bw.tap(i - 1));
    P2LGConv d = gconv_desc(B, L.h[i], L.w[i], kCout[i], kCin[i], 3, 1, 1);
    RET_IF(p2l_gconv_fwd(&d, ga, v->wt[i], nullptr, nullptr, nullptr, gtap, Wk + L.y[i - 1], gb, st));
    float* t = ga; ga = gb; gb = t;
  }
  // conv2 -> pooled relu2 -> relu2 (+ tap) -> conv1 ...
  {
    P2LGConv d = gconv_desc(B, L.h[2], L.w[2], kCout[2], kCin[2], 3, 1, 1);
    RET_IF(p2l_gconv_fwd(&d, ga, v->wt[2], nullptr, nullptr, nullptr, nullptr, nullptr, gb, st));
    RET_IF(bw.tap(1));
    RET_IF(p2l_maxpool3s2_bwd(Wk + L.y[1], gb, gtap, ga, B, L.h[1], L.w[1], 192, st));
  }
  {
    P2LGConv d = gconv_desc(B, L.h[1], L.w[1], kCout[1], kCin[1], 5, 1, 2);
    RET_IF(p2l_gconv_fwd(&d, ga, v->wt[1], nullptr, nullptr, nullptr, nullptr, nullptr, gb, st));
    RET_IF(bw.tap(0));
    RET_IF(p2l_maxpool3s2_bwd(Wk + L.y[0], gb, gtap, ga, B, L.h[0], L.w[0], 64, st));
  }
  RET_IF(p2l_conv1_dgrad(ga, v->wt[0], dimg16, B, H, W, 64, 11, 4, 2, st));
  return loss_bwd_end(bw);
}
