// ProjectionLoss / PerceptualLoss with the LPIPS-SqueezeNet network (round 6).  The reference passes any lpips net
// name through (pix2latent/loss_functions.py:128-131 `lpips.LPIPS(net=net, spatial=True)`); 'squeeze' was the one
// of the three lpips ships that had no native plan.  torchvision squeezenet1_1.features as
// lpips.pretrained_networks.squeezenet slices it [3P-recall]:
//   conv(3,64,k3,s2) relu | pool fire(64,16,64) fire(128,16,64) | pool fire(128,32,128) fire(256,32,128) |
//   pool fire(256,48,192) | fire(384,48,192) | fire(384,64,256) | fire(512,64,256)         (7 taps)
//   Fire(in, s, e): x -> q = relu(conv1x1(in, s)) -> cat(relu(conv1x1(s, e)), relu(conv3x3(s, e, pad 1)))
//   pool = 3x3 stride-2 max-pool with ceil_mode: for the image sizes this plan accepts every window is whole
//   ((n - 3) even at each of the three pools: all powers of two >= 64), so it is p2l_maxpool3s2.
// Same structure as the AlexNet plan (p2l_plan_alex.hip): the generic gather conv (p2l_gconv_fwd, exact fp32
// MFMA), target features / adjoint-resized weight maps cached per target, weighted spatial sum at tap
// resolution, dgrad-only backward with fixed-order reductions.  The two expand branches of a fire write the two
// channel halves of one tensor; their input gradients meet in one launch (the second takes the first as residual
// and applies the squeeze ReLU's mask).
#include "p2l_loss_shell.h"

namespace {

constexpr int NF = 8, NT = 7;
const int kIn[NF] = {64, 128, 128, 256, 256, 384, 384, 512};
const int kSq[NF] = {16, 16, 32, 32, 48, 48, 64, 64};
const int kEx[NF] = {64, 64, 128, 128, 192, 192, 256, 256};
const int kStage[NF] = {0, 0, 1, 1, 2, 2, 2, 2};       // which pooled grid a fire runs on
const int kTapOfFire[NF] = {-1, 1, -1, 2, 3, 4, 5, 6};  // LPIPS tap its output is (tap 0 = relu(conv0))
const int kTapC[NT] = {64, 128, 256, 384, 384, 512, 512};

struct SqLayout : LossLayout {
  int h0, w0;              // conv0 output grid
  int h[3], w[3];          // the three pooled grids
  size_t y0, p[3], q[NF], out[NF];
  size_t gq, gq2;          // backward scratch of a fire's squeeze output
};

int pool_ok(int n) { return n >= 3 && ((n - 3) & 1) == 0; }

int sq_layout(int B, int H, int W, SqLayout& L) {
  if (B < 1 || H < 35 || W < 35) return P2L_EINVAL;
  L.h0 = (H - 3) / 2 + 1; L.w0 = (W - 3) / 2 + 1;
  int hh = L.h0, ww = L.w0;
  for (int s = 0; s < 3; ++s) {
    // ceil_mode pools: only sizes whose last window is whole (floor == ceil) are taken
    if (!pool_ok(hh) || !pool_ok(ww)) return P2L_EINVAL;
    hh = (hh - 3) / 2 + 1; ww = (ww - 3) / 2 + 1;
    L.h[s] = hh; L.w[s] = ww;
  }
  Arena a;
  size_t max_act = (size_t)B * L.h0 * L.w0 * 64;
  L.y0 = a.take(max_act);
  const int pc[3] = {64, 128, 256};
  for (int s = 0; s < 3; ++s) L.p[s] = a.take((size_t)B * L.h[s] * L.w[s] * pc[s]);
  size_t max_q = 0;
  for (int i = 0; i < NF; ++i) {
    const size_t px = (size_t)B * L.h[kStage[i]] * L.w[kStage[i]];
    L.q[i] = a.take(px * kSq[i]);
    L.out[i] = a.take(px * 2 * kEx[i]);
    if (px * 2 * kEx[i] > max_act) max_act = px * 2 * kEx[i];
    if (px * kIn[i] > max_act) max_act = px * kIn[i];
    if (px * kSq[i] > max_q) max_q = px * kSq[i];
  }
  LossTaps& T = L.taps;
  T.n = NT;
  T.h[0] = L.h0; T.w[0] = L.w0; T.y[0] = L.y0;
  for (int i = 0; i < NF; ++i)
    if (kTapOfFire[i] >= 0) {
      const int k = kTapOfFire[i];
      T.h[k] = L.h[kStage[i]]; T.w[k] = L.w[kStage[i]]; T.y[k] = L.out[i];
    }
  for (int k = 0; k < NT; ++k) T.C[k] = kTapC[k];
  L.tail.take(a, B, H, W, T, max_act);
  L.gq = a.take(max_q);
  L.gq2 = a.take(max_q);
  L.total = a.off;
  return P2L_OK;
}

// SqueezeNet1.1 features on an NHWC16 image: y0 = relu(conv0), q[i] / out[i] per fire, p[s] pooled inputs
int sq_forward(const P2LSqueezeLpips* v, const float* img16, int B, int H, int W, float* Wk, const SqLayout& L,
               void* st) {
  {
    P2LGConv d = gconv_desc(B, H, W, 16, 64, 3, 2, 0);
    d.relu = 1;
    RET_IF(p2l_gconv_fwd(&d, img16, v->w0, v->b0, v->in_s, v->in_t, nullptr, nullptr, Wk + L.y0, st));
  }
  const float* x = Wk + L.y0;
  int xh = L.h0, xw = L.w0;
  for (int i = 0; i < NF; ++i) {
    const int s = kStage[i], h = L.h[s], w = L.w[s];
    if (i == 0 || kStage[i - 1] != s) {                // a pool in front of the first fire of a stage
      RET_IF(p2l_maxpool3s2_fwd(x, Wk + L.p[s], B, xh, xw, kIn[i], st));
      x = Wk + L.p[s]; xh = h; xw = w;
    }
    {
      P2LGConv d = gconv_desc(B, h, w, kIn[i], 64, 1, 1, 0);   // squeeze: output channels padded to 64, sq stored
      d.relu = 1; d.n_store = kSq[i]; d.y_ld = kSq[i];
      RET_IF(p2l_gconv_fwd(&d, x, v->sq_w[i], v->sq_b[i], nullptr, nullptr, nullptr, nullptr, Wk + L.q[i], st));
    }
    {
      P2LGConv d = gconv_desc(B, h, w, kSq[i], kEx[i], 1, 1, 0);
      d.relu = 1; d.y_ld = 2 * kEx[i];
      RET_IF(p2l_gconv_fwd(&d, Wk + L.q[i], v->e1_w[i], v->e1_b[i], nullptr, nullptr, nullptr, nullptr,
                           Wk + L.out[i], st));
    }
    {
      P2LGConv d = gconv_desc(B, h, w, kSq[i], kEx[i], 3, 1, 1);
      d.relu = 1; d.y_ld = 2 * kEx[i];
      RET_IF(p2l_gconv_fwd(&d, Wk + L.q[i], v->e3_w[i], v->e3_b[i], nullptr, nullptr, nullptr, nullptr,
                           Wk + L.out[i] + kEx[i], st));
    }
    x = Wk + L.out[i];
  }
  return P2L_OK;
}

}  // namespace

extern "C" size_t p2l_sqz_cache_floats(int B, int H, int W, size_t nft_off[7], size_t wt_off[7],
                                       size_t* wsum_off) {
  SqLayout L;
  if (sq_layout(B, H, W, L)) return 0;
  return loss_cache_floats(L.taps, B, nft_off, wt_off, wsum_off);
}

// test hook (include/p2l_test.h): idx 0 = relu(conv0), 1..8 = the squeeze outputs q of fires 0..7,
// 9..16 = the (concatenated) outputs of fires 0..7; NHWC
extern "C" int p2l_sqzloss_ws_lookup(int B, int H, int W, int idx, size_t* float_off, int32_t shape[4]) {
  if (idx < 0 || idx > 2 * NF || !float_off || !shape) return P2L_EINVAL;
  SqLayout L;
  RET_IF(sq_layout(B, H, W, L));
  shape[0] = B;
  if (idx == 0) {
    *float_off = L.y0; shape[1] = L.h0; shape[2] = L.w0; shape[3] = 64;
    return P2L_OK;
  }
  const int i = (idx - 1) % NF, s = kStage[i];
  shape[1] = L.h[s]; shape[2] = L.w[s];
  if (idx <= NF) { *float_off = L.q[i]; shape[3] = kSq[i]; }
  else { *float_off = L.out[i]; shape[3] = 2 * kEx[i]; }
  return P2L_OK;
}

extern "C" size_t p2l_sqzloss_ws_bytes(int B, int H, int W) {
  SqLayout L;
  if (sq_layout(B, H, W, L)) return 0;
  return L.total * sizeof(float);
}

extern "C" int p2l_sqzloss_prepare(const P2LSqueezeLpips* v, const float* target, const float* weight,
                                   const float* loss_mask, int B, int H, int W, const P2LLossCache7* cache,
                                   void* ws, size_t ws_bytes, void* st) {
  SqLayout L;
  RET_IF(sq_layout(B, H, W, L));
  L.taps.bind(v, cache);
  return loss_prepare(L, target, weight, loss_mask, B, H, W, ws, ws_bytes, st,
                      [&](const float* x) { return sq_forward(v, x, B, H, W, (float*)ws, L, st); });
}

extern "C" int p2l_sqzloss_fwd(const P2LSqueezeLpips* v, const float* img16, const float* target,
                               const float* weight, const float* loss_mask, const P2LLossCache7* cache,
                               float beta, int use_lpips, int B, int H, int W, void* ws, size_t ws_bytes,
                               float* loss, float* loss_l1, float* loss_lpips, void* st) {
  SqLayout L;
  RET_IF(sq_layout(B, H, W, L));
  L.taps.bind(v, cache);
  return loss_fwd(L, img16, target, weight, loss_mask, beta, use_lpips, B, H, W, ws, ws_bytes, loss, loss_l1,
                  loss_lpips, st, [&](const float* x) { return sq_forward(v, x, B, H, W, (float*)ws, L, st); });
}

extern "C" int p2l_sqzloss_bwd(const P2LSqueezeLpips* v, const float* img16, const float* target,
                               const float* weight, const float* loss_mask, const P2LLossCache7* cache,
                               float beta, int use_lpips, const float* gloss, int B, int H, int W, void* ws,
                               size_t ws_bytes, float* dimg16, void* st) {
  SqLayout L;
  RET_IF(sq_layout(B, H, W, L));
  L.taps.bind(v, cache);
  LossBwd bw;
  RET_IF(loss_bwd_begin(L, img16, target, weight, loss_mask, beta, use_lpips, gloss, B, H, W, ws, ws_bytes, dimg16,
                        st, bw));
  if (bw.done) return P2L_OK;
  float* Wk = (float*)ws;
  float *ga = bw.ga, *gb = bw.gb, *gtap = bw.gtap;   // ga = M_i: fire i's PRE-ReLU output gradient (both halves)
  float* gq = Wk + L.gq;
  float* gq2 = Wk + L.gq2;
  // the last fire's output is consumed by its tap only
  RET_IF(bw.tap(6));
  {
    const int i = NF - 1, C2 = 2 * kEx[i];
    RET_IF(p2l_relu_mask(Wk + L.out[i], C2, gtap, C2, ga, C2, (int64_t)B * L.h[2] * L.w[2], C2, st));
  }
  for (int i = NF - 1; i >= 0; --i) {
    const int s = kStage[i], h = L.h[s], w = L.w[s], C2 = 2 * kEx[i];
    // d q = dgrad(expand1x1)(M[:, :ex]) + dgrad(expand3x3)(M[:, ex:]), then the squeeze ReLU's mask
    {
      P2LGConv d = gconv_desc(B, h, w, kEx[i], 64, 1, 1, 0);
      d.x_ld = C2; d.n_store = kSq[i]; d.y_ld = kSq[i];
      RET_IF(p2l_gconv_fwd(&d, ga, v->e1_wt[i], nullptr, nullptr, nullptr, nullptr, nullptr, gq, st));
    }
    {
      P2LGConv d = gconv_desc(B, h, w, kEx[i], 64, 3, 1, 1);
      d.x_ld = C2; d.n_store = kSq[i]; d.y_ld = kSq[i]; d.res_ld = kSq[i]; d.mask_ld = kSq[i];
      RET_IF(p2l_gconv_fwd(&d, ga + kEx[i], v->e3_wt[i], nullptr, nullptr, nullptr, gq, Wk + L.q[i], gq2, st));
    }
    // d x = dgrad(squeeze)(d q): the gradient w.r.t. the fire's input tensor
    const bool pooled_in = (i == 0 || kStage[i - 1] != s);
    const int tk = (i > 0) ? kTapOfFire[i - 1] : 0;      // tap on the tensor in front (fire i-1's output | y0)
    if (tk >= 0) RET_IF(bw.tap(tk));
    P2LGConv d = gconv_desc(B, h, w, kSq[i], kIn[i], 1, 1, 0);
    if (!pooled_in) {
      // the input IS fire i-1's output: + its tap gradient, x its ReLU mask, in the same launch
      RET_IF(p2l_gconv_fwd(&d, gq2, v->sq_wt[i], nullptr, nullptr, nullptr, tk >= 0 ? gtap : nullptr,
                           Wk + L.out[i - 1], gb, st));
    } else {
      // the input is the pooled tensor: gradient to it, then pool backward + tap gradient + ReLU mask in one pass
      RET_IF(p2l_gconv_fwd(&d, gq2, v->sq_wt[i], nullptr, nullptr, nullptr, nullptr, nullptr, gb, st));
      const float* src = (i == 0) ? Wk + L.y0 : Wk + L.out[i - 1];
      const int sh = (i == 0) ? L.h0 : L.h[s - 1], sw = (i == 0) ? L.w0 : L.w[s - 1];
      RET_IF(p2l_maxpool3s2_bwd(src, gb, tk >= 0 ? gtap : nullptr, ga, B, sh, sw, kIn[i], st));
      float* t = ga; ga = gb; gb = t;                    // (result in the old ga: swap so that it is `gb` below)
    }
    float* t = ga; ga = gb; gb = t;                      // M_{i-1} (or the masked gradient of y0) is now `ga`
  }
  RET_IF(p2l_conv1_dgrad(ga, v->wt0, dimg16, B, H, W, 64, 3, 2, 0, st));
  return loss_bwd_end(bw);
}
