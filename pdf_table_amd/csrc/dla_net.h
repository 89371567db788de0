// dla_net.h -- the DLA-34 base (center_net/modeling_centernet.py:274-402: DLA.forward :382-402, Tree.forward :259-271, Root
// :167-175, BasicBlock :58-72) as launches on the engine's kernels, shared by the two table-structure detectors built on it:
// Lore's DLASeg (lore_model.hip: DCN up-sampling) and CenterNet's (centernet_model.hip: plain 1x1 / 3x3 up-sampling).
// Included by one translation unit each; everything here is internal to it.
#pragma once

#include <stdlib.h>

#include <string>
#include <vector>

#include "net_ctx.h"

namespace PT_FMT_NS {

int pt_launch_conv3x3_c16(pt_engine* e, const bf16_t* in, const bf16_t* w, const float* bias, bf16_t* out, int B, int H, int W,
                          int N, int stride, int split, hipStream_t s);
int pt_launch_dla_thin_chain(pt_engine* e, const bf16_t* in, int B, int H, int W, const bf16_t* w_stem, const float* b_stem, const bf16_t* w0,
                             const float* b0, const bf16_t* w1, const float* b1, bf16_t* out, hipStream_t s);

namespace {

struct DlaCtx : NetCtx {
  bf16_t* cols = nullptr;   // shared DCN column scratch (largest site)
  float* om = nullptr;      // shared offset/mask scratch, fp32 [pixel][32]
  const int* ylimit = nullptr;   // when set: convs skip output tiles at rows >= *ylimit (sparse-head mosaics)
  double alg_scale = 1.0;        // roofline accounting: fraction of a launch's output pixels the algorithm needs
  // a part of a batch run on its own (Lore's row bands: one tall image of part_H input rows cut from pick_n maps of whole_H rows): the conv launcher
  // chooses its kernels as for the whole batch (ConvDesc.pick_B / pick_Ho), so that a value is summed in the same order wherever it is computed
  int pick_n = 0, part_H = 0, whole_H = 0;
  void pick(ConvDesc& c) const {
    if (!pick_n) return;
    const int in_h = (int)((long long)c.H * whole_H / part_H), pad = c.ks / 2;
    c.pick_B = pick_n;
    c.pick_Ho = (in_h + 2 * pad - c.ks) / c.stride + 1;
  }

  // conv with folded bias; q = weight name prefix; N = GEMM width (multiple of 64), nv = channels stored (0 = N)
  void conv(const T& in, const std::string& q, int N, int ks, int stride, const T& out, int relu, const T* res = nullptr,
            int nv = 0, float* out_f32 = nullptr, int f32_cs = 0, int cin_override = 0, int alg_n = 0) {
    ConvDesc c;
    if (!conv_desc(c, in, q, N, ks, stride, relu)) return;
    if (cin_override) c.Cin = cin_override;
    c.n_valid = nv; c.ylimit = ylimit; c.alg_n = alg_n; c.alg_scale = alg_scale;
    pick(c);
    if (out_f32) to_f32(c, out_f32, f32_cs);
    else to_map(c, out);
    if (res) { c.res = res->p; c.res_mode = 1; }
    launch(c);
  }
  // 1x1 conv over the channel concatenation of `ins` (never materialised): one GEMM whose K walks the tensors
  void conv_cat(const std::vector<T>& ins, const std::string& q, int N, const T& out, int relu) {
    const PtTensor* w = get(q + (x3 ? ".w3" : ".w"));
    const PtTensor* b = get(q + ".b");
    if (!go()) return;
    ConvDesc c;
    c.in = ins[0].p; c.B = n; c.H = ins[0].H; c.W = ins[0].W;
    c.nseg = (int)ins.size();
    c.Cin = 0;
    for (int i = 0; i < c.nseg; ++i) {
      c.seg_c[i] = ins[i].C;
      c.Cin += ins[i].C;
      if (i) c.in_more[i - 1] = ins[i].p;
    }
    c.w = W(w); c.bias = F(b);
    c.N = N; c.ks = 1; c.stride = 1; c.relu = relu; c.split = x3; c.alg_scale = alg_scale;
    pick(c);
    to_map(c, out);
    launch(c);
  }
  T maxpool2(const T& x) {
    T o = alloc(x.H / 2, x.W / 2, x.C);
    if (go()) {
      e->prof.next_bytes = (double)n * x.H * x.W * x.C * 2.0 * mul * 1.25;
      PtProfScope ps(e, s, PT_PROF_OTHER, 0, "maxpool2x2");
      const int r = pt_launch_maxpool_kxk(x.p, n, x.H, x.W, x.C, 2, 2, 0, x3, o.p, s);
      if (r != PT_OK) rc = r;
    }
    return o;
  }
  T block(const std::string& q, const T& x, const T& residual, int stride, int cout) {
    T t = alloc(x.H / stride, x.W / stride, cout);
    conv(x, q + ".conv1", cout, 3, stride, t, 1);
    T o = alloc(t.H, t.W, cout);
    conv(t, q + ".conv2", cout, 3, 1, o, 1, &residual);
    return o;
  }
  // pooled: MaxPool2d(stride)(x) when the caller already holds it (the outer tree of a two-level stage pools the same x with the same stride)
  T tree(const std::string& q, int levels, const T& x, int cin, int cout, int stride, bool level_root,
         std::vector<T> children, const T* pooled = nullptr) {
    T bottom = stride > 1 ? (pooled ? *pooled : maxpool2(x)) : x;
    if (level_root) children.push_back(bottom);
    if (levels == 1) {
      T residual = bottom;
      if (cin != cout) {
        residual = alloc(bottom.H, bottom.W, cout);
        conv(bottom, q + ".project", cout, 1, 1, residual, 0);
      }
      T x1 = block(q + ".tree1", x, residual, stride, cout);
      T x2 = block(q + ".tree2", x1, x1, 1, cout);
      std::vector<T> ins = {x2, x1};
      ins.insert(ins.end(), children.begin(), children.end());
      T o = alloc(x1.H, x1.W, cout);
      conv_cat(ins, q + ".root", cout, o, 1);      // Root: conv(cat(x2, x1, *children)) + BN + ReLU, one launch
      return o;
    }
    // tree1 has this tree's input and stride: it takes `bottom` for its residual instead of pooling x again (the maximum is exact: same bits).
    // PT_DLA_POOL_ONCE=0: the second launch (A/B switch, read per call)
    const char* once_env = getenv("PT_DLA_POOL_ONCE");
    const bool once = stride > 1 && !(once_env && atoi(once_env) == 0);
    T x1 = tree(q + ".tree1", levels - 1, x, cin, cout, stride, false, {}, once ? &bottom : nullptr);
    children.push_back(x1);
    return tree(q + ".tree2", levels - 1, x1, cout, cout, 1, false, children);
  }
};

// The front segment of DLA.forward: base_layer, level0, level1, level2 on c.n images of H x W.  Its layers have small static receptive fields:
// kFront lists them (kernel, stride, padding) along the longest path to a level-2 output row -- level2's tree1.conv1 (stride 2), then tree1.conv2,
// tree2.conv1, tree2.conv2; the 2x2 pool, the 1x1 project and the 1x1 root reach no farther -- and dla_front_radius() folds the list into the
// distance, in input rows, beyond which an input row cannot reach a given row of `layers[2]` (the stride-4 map; row r sits at input row 4 r)
struct DlaFrontLayer { int k, stride, pad; };
constexpr DlaFrontLayer kFront[] = {{7, 1, 3},                              // base_layer
                                    {3, 1, 1},                              // level0
                                    {3, 2, 1},                              // level1
                                    {3, 2, 1}, {3, 1, 1}, {3, 1, 1}, {3, 1, 1}};   // level2: tree1.conv1, tree1.conv2, tree2.conv1, tree2.conv2
constexpr int kFrontStride = 4;
constexpr int dla_front_radius() {
  // output row 0 reads input rows [lo, hi]: walk the list backwards
  int lo = 0, hi = 0;
  for (int i = (int)(sizeof(kFront) / sizeof(kFront[0])) - 1; i >= 0; --i) {
    lo = lo * kFront[i].stride - kFront[i].pad;
    hi = hi * kFront[i].stride - kFront[i].pad + kFront[i].k - 1;
  }
  return hi > -lo ? hi : -lo;
}
static_assert(dla_front_radius() == 19, "DLA-34 front segment: receptive-field radius");

static void dla34_front(DlaCtx& c, std::vector<T>& layers, const bf16_t* x, int H, int W) {
  pt_engine* e = c.e;
  hipStream_t s = c.s;
  const int n = c.n;
  const int ch[6] = {16, 32, 64, 128, 256, 512};
  const int lv[6] = {1, 1, 1, 2, 2, 1};
  // bf16 mode: base_layer -> level0 -> level1 in one launch, the two full-resolution 16-channel maps never leave the CU
  // (lore_kernels.hip: dla_thin_chain_kernel; PT_DLA_CHAIN=0: the three launches, A/B switch read per call)
  const char* chain_env = getenv("PT_DLA_CHAIN");
  const bool chain = !c.x3 && H % 2 == 0 && W % 2 == 0 && !(chain_env && atoi(chain_env) == 0);
  if (chain) {
    layers[1] = c.alloc(H / 2, W / 2, 32);
    const PtTensor *ws = c.get("base_layer.w"), *bs = c.get("base_layer.b"), *w0 = c.get("level0.wt"), *b0 = c.get("level0.bt"),
                   *w1 = c.get("level1.wt"), *b1 = c.get("level1.bt");
    if (c.go()) {
      const int r = pt_launch_dla_thin_chain(e, x, n, H, W, c.W(ws), c.F(bs), c.W(w0), c.F(b0), c.W(w1), c.F(b1), layers[1].p, s);
      if (r != PT_OK) c.rc = r;
    }
  } else {
    T t0 = c.alloc(H, W, 16);
    const PtTensor* w = c.get(c.x3 ? "base_layer.w3" : "base_layer.w");
    const PtTensor* b = c.get("base_layer.b");
    if (c.go()) {
      const int r = pt_launch_stem7x7(e, x, n, H, W, c.W(w), c.F(b), t0.p, c.x3, s, 1, 16);
      if (r != PT_OK) c.rc = r;
    }
    layers[0] = c.alloc(H, W, 16);
    layers[1] = c.alloc(H / 2, W / 2, 32);
    for (int lv1 = 0; lv1 < 2; ++lv1) {
      const std::string q = lv1 ? "level1" : "level0";
      const PtTensor* w = c.get(q + (c.x3 ? ".wt3" : ".wt"));
      const PtTensor* b = c.get(q + ".bt");
      if (c.go()) {
        const int r = pt_launch_conv3x3_c16(e, lv1 ? layers[0].p : t0.p, c.W(w), c.F(b), layers[lv1].p, n, H, W, lv1 ? 32 : 16,
                                            lv1 ? 2 : 1, c.x3, s);
        if (r != PT_OK) c.rc = r;
      }
    }
  }
  layers[2] = c.tree("level2", lv[2], layers[1], ch[1], ch[2], 2, false, {});
}

// levels 3 .. 5 behind a front segment
static void dla34_rest(DlaCtx& c, std::vector<T>& layers) {
  const int ch[6] = {16, 32, 64, 128, 256, 512};
  const int lv[6] = {1, 1, 1, 2, 2, 1};
  for (int l = 3; l < 6; ++l)
    layers[l] = c.tree("level" + std::to_string(l), lv[l], layers[l - 1], ch[l - 1], ch[l], 2, true, {});
}

// DLA.forward up to level5: layers[l] = output of level l (levels 0 and 1 only as far as the chosen path materialises them)
static std::vector<T> dla34_base(DlaCtx& c, const bf16_t* x, int H, int W) {
  std::vector<T> layers(6);
  dla34_front(c, layers, x, H, W);
  dla34_rest(c, layers);
  return layers;
}

}  // namespace

}  // namespace PT_FMT_NS
