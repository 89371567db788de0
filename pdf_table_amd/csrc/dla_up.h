// dla_up.h -- the plain DLAUp / IDAUp up-path (1x1 projections, depthwise ConvTranspose2d up-samplers, 3x3 nodes over a channel concat) as launches
// on the engine's kernels, shared by the two DLASeg graphs that use it: CenterNet's table-cell detector (centernet_model.hip) and DocXLayout's layout
// detector (docx_model.hip).  How the concat is laid out is told at the top of centernet_model.hip.  Included by one translation unit per model;
// everything here is internal to it.
#pragma once

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

}  // namespace PT_FMT_NS
