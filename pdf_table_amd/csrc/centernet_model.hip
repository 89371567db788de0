// centernet_model.hip -- launch graph of CenterNet's table-cell detector (Cycle-CenterNet: DLA-34 base + DLAUp + four heads).
//
// Reference graph: DLASeg.forward center_net/modeling_centernet.py:655-661 (TableStructureRec, modeling_table_structure.py:22-47)
//   base    = dla34 (the same DLA as Lore's, dla_net.h)
//   dla_up  = DLAUp.forward :591-599 over IDAUp.forward :550-565, channels [64,128,256,512], scales [1,2,4,8]:
//             ida_0 (256 ch) on levels 4..5, ida_1 (128 ch) on 3..5, ida_2 (64 ch) on 2..5, every up factor 2.  An IDAUp projects
//             each input with conv1x1 + BN + ReLU (unless it already has out_dim channels), up-samples it with a depthwise
//             ConvTranspose2d(4, stride 2, pad 1), and its node i is conv3x3(cat([x, layer_i])) + BN + ReLU -- a concatenation,
//             not Lore's DCN on a sum
//   heads   = conv3x3(64->256) + bias + ReLU, conv1x1 -> k + bias for hm (2), v2c (8), c2v (8), reg (2)
// Engine mapping: the concat a node reads is one 2C-channel map that its producers write in halves -- the up-sampler into channel
// slice [C, 2C) (dwconvt_up2_add_kernel's SLICE form), the previous node's conv epilogue into [0, C) through out_coff and the
// output channel stride.  The first half of an IDAUp's first node is a base level that other launches also read densely: it is
// copied in.  A node output that the next IDAUp projects is needed as a dense map as well (the 1x1 GEMM reads channel stride ==
// Cin): ida_1's node_1 is written into the concat and copied out.
#include "dla_net.h"

namespace PT_FMT_NS {

int pt_launch_dwconvt_up2_slice(const bf16_t* in, const float* w, bf16_t* out, int out_cstride, int out_coff, int out_lo_off, int B,
                                int h, int wd, int C, int split, hipStream_t s);

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

inline unsigned cn_grid(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);     // grid-stride loop beyond that
}

// dst[pixel][half * dlo + c] = src[pixel][half * slo + c] for c < C and half < (split ? 2 : 1), 8 channels (16 bytes) per thread
__global__ __launch_bounds__(256) void cn_copy_slice_kernel(const bf16_t* __restrict__ src, int scs, int slo, bf16_t* __restrict__ dst,
                                                            int dcs, int dlo, long long npix, int C, int split) {
  a16_kernel_enter();
  const int cg = C >> 3;
  const int G = split ? 2 * cg : cg;
  const long long total = npix * G;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long pix = i / G;
    const int g = (int)(i - pix * G);
    const int half = g >= cg ? 1 : 0;
    const int c = (g - half * cg) * 8;
    *reinterpret_cast<u32x4*>(dst + pix * dcs + half * dlo + c) = *reinterpret_cast<const u32x4*>(src + pix * scs + half * slo + c);
  }
}

struct Slice {          // a channel slice of a map: pixel stride cs, (hi | lo) distance lo, first channel at p
  bf16_t* p = nullptr;
  int cs = 0, lo = 0;
};

struct CCtx : DlaCtx {
  Slice dense(const T& t) const { return Slice{t.p, t.C * mul, t.C}; }
  Slice half(const T& cat, int which) const { return Slice{cat.p ? cat.p + which * (cat.C / 2) : nullptr, cat.C * mul, cat.C}; }

  void copy(const T& like, const Slice& from, const Slice& to) {
    if (!go()) return;
    const long long npix = (long long)n * like.H * like.W;
    e->prof.next_bytes = (double)npix * like.C * 2.0 * mul * 2.0;
    PtProfScope ps(e, s, PT_PROF_OTHER, 0, "centernet concat copy");
    hipLaunchKernelGGL(cn_copy_slice_kernel, dim3(cn_grid(npix * (like.C / 8) * mul)), dim3(256), 0, s, from.p, from.cs, from.lo, to.p,
                       to.cs, to.lo, npix, like.C, x3);
    if (hipGetLastError() != hipSuccess) {
      pt_set_error("centernet concat copy: launch failed");
      rc = PT_ERR_HIP;
    }
  }
  // conv + folded bias (+ ReLU) into a slice of a wider map
  void conv_into(const T& in, const std::string& q, int N, int ks, const Slice& out, int relu) {
    ConvDesc c;
    if (!conv_desc(c, in, q, N, ks, 1, relu)) return;
    c.alg_scale = alg_scale;
    c.out = out.p; c.out_cstride = out.cs; c.out_lo_off = out.lo;
    launch(c);
  }
  // IDAUp.forward on layers[startp .. endp); keep_dense: the node outputs are projected by the next IDAUp
  void ida(const std::string& q, std::vector<T>& layers, int startp, int endp, int o, bool keep_dense) {
    const T& x0 = layers[startp];
    T cat = alloc(x0.H, x0.W, 2 * o);
    copy(x0, dense(x0), half(cat, 0));
    for (int i = startp + 1; i < endp; ++i) {
      const std::string js = std::to_string(i - startp);
      T p = layers[i];
      if (p.C != o) {
        p = alloc(layers[i].H, layers[i].W, o);
        conv(layers[i], q + ".proj_" + js, o, 1, 1, p, 1);
      }
      const PtTensor* wu = get(q + ".up_" + js + ".wf32");
      if (go()) {
        e->prof.next_bytes = (double)n * p.H * p.W * o * 2.0 * mul * 5.0;      // in once, out at 2 x 2 the pixels
        char label[48];
        snprintf(label, sizeof(label), "dw convT up %d @%dx%d", o, p.H * 2, p.W * 2);
        PtProfScope ps(e, s, PT_PROF_OTHER, 0, label);
        const Slice u = half(cat, 1);
        const int r = pt_launch_dwconvt_up2_slice(p.p, F(wu), cat.p, u.cs, o, u.lo, n, p.H, p.W, o, x3, s);
        if (r != PT_OK) rc = r;
      }
      const bool last = i + 1 == endp;
      if (last) {
        T y = alloc(cat.H, cat.W, o);
        conv_into(cat, q + ".node_" + js, o, 3, dense(y), 1);
        layers[i] = y;
      } else {
        T next = alloc(cat.H, cat.W, 2 * o);
        conv_into(cat, q + ".node_" + js, o, 3, half(next, 0), 1);
        if (keep_dense) {      // also projected by the next IDAUp: materialised
          T y = alloc(cat.H, cat.W, o);
          copy(y, half(next, 0), dense(y));
          layers[i] = y;
        } else {
          layers[i] = T();     // read by the next node only, through the concat
        }
        cat = next;
      }
    }
  }
};

}  // namespace

// x: NHWC4 bf16 [n, H, W, 4] ([hi rgb0 | lo rgb0] in BF16X3 mode); heads: fp32 NHWC at H/4 x W/4, channel stride 8 each
// (hm: 2 valid, v2c: 8, c2v: 8, reg: 2 valid)
int pt_centernet_net(pt_engine* e, const bf16_t* x, int n, int H, int W, float* hm, float* v2c, float* c2v, float* reg, hipStream_t s) {
  PT_REQUIRE(H % 32 == 0 && W % 32 == 0 && H > 0 && W > 0, "CenterNet net: input %dx%d must be multiples of 32", H, W);
  PT_REQUIRE(x && n > 0 && hm && v2c && c2v && reg, "CenterNet net: null pointer");
  const PtModel* m = pt_find_model(e, PT_MODEL_CENTERNET_DLA34, "CenterNet DLA-34", "PT_MODEL_CENTERNET_DLA34");
  if (!m) return PT_ERR_STATE;
  CCtx c;
  c.init(e, m, "CenterNet DLA-34", s, n, PT_ARENA_TSR);
  float* heads[4] = {hm, v2c, c2v, reg};
  const char* hname[4] = {"hm", "v2c", "c2v", "reg"};
  const int hreal[4] = {2, 8, 8, 2};
  return pt_plan_then_launch(c, "CenterNet net", [&] {
    std::vector<T> layers = dla34_base(c, x, H, W);
    // DLAUp.forward: ida_0 on [4,6), ida_1 on [3,6), ida_2 on [2,6); each replaces layers[startp + 1 ..] by its node outputs
    c.ida("dla_up.ida_0", layers, 4, 6, 256, true);
    c.ida("dla_up.ida_1", layers, 3, 6, 128, true);
    c.ida("dla_up.ida_2", layers, 2, 6, 64, false);
    const T feat = layers[5];
    T hid = c.alloc(feat.H, feat.W, 256);
    for (int h = 0; h < 4; ++h) {
      c.conv(feat, std::string(hname[h]) + ".0", 256, 3, 1, hid, 1);
      c.conv(hid, std::string(hname[h]) + ".2", 64, 1, 1, T(), 0, nullptr, 8, heads[h], 8, 0, hreal[h]);
    }
    return c.rc;
  });
}

}  // namespace PT_FMT_NS
