// lore_model.hip -- launch graph of Lore's table-cell detector (DLA-34 backbone + DCN up-sampling + six heads).
//
// Reference graph: DLASeg.forward lore/lore_dla_34.py:184-196
//   base    = dla34: DLA.forward center_net/modeling_centernet.py:382-402 (Tree.forward :259-271, Root :167-175,
//             BasicBlock :58-72)
//   dla_up  = DLAUp.forward :128-134 over IDAUp.forward :106-112; every proj/node is DeformConv :65-83 =
//             DCN (lore/dcnv2.py:71-86) -> BN -> ReLU; every up is a depthwise ConvTranspose2d
//   heads   = conv3x3(64->256)+ReLU+conv1x1 for hm, st, wh, ax, cr, reg (:159-182)
// Engine mapping: Conv+BN(+ReLU) folded, residual add in the conv epilogue; Root's conv over a channel concat is
// evaluated child by child, accumulating through the residual path (no concat tensor); DCN = offset/mask conv (fp32
// out) -> dcn_im2col_kernel -> 1x1 GEMM over 9*C columns; the `up(x) + skip` add is fused into the up-sampler.
// The 16-channel levels (base_layer, level0, level1) run on dedicated thin kernels and keep their real 16 channels.
// The base and the launch context it runs on are shared with CenterNet's detector (dla_net.h).
#include <math.h>
#include <string.h>

#include "dla_net.h"

namespace PT_FMT_NS {

// ---------------------------------------------------------------------------------------------------------------------
// Row bands of the front segment (include/pdftable_hip.h: pt_tsr_plan_bands).  The radius comes from dla_net.h's layer list.
// ---------------------------------------------------------------------------------------------------------------------
int pt_lore_band_radius() { return dla_front_radius(); }

constexpr int kBandSlack = 2;               // rows added to the content on either side before anything else
constexpr int kBandStackCap = 32768;        // input rows per stack: the largest map of the segment (32 channels at half size) is then 512 MiB

int pt_lore_plan_bands(const pt_tsr_table* tabs, int n, int inp_h, int inp_w, int max_stack_rows, int margin, pt_tsr_band* out, int* n_stacks,
                       double* row_fraction) {
  PT_REQUIRE(tabs && out && n > 0 && inp_h > 0 && inp_w > 0 && inp_h % kFrontStride == 0, "tsr band plan: bad arguments");
  const int R = margin < 0 ? dla_front_radius() : margin, AL = PT_TSR_BAND_ALIGN;
  const int cap = (max_stack_rows <= 0 || max_stack_rows > kBandStackCap) ? kBandStackCap : max_stack_rows;
  auto sat = [](double v) { return (long long)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); };
  int stack = -1, used = 0;
  long long planned = 0;
  for (int t = 0; t < n; ++t) {
    const pt_tsr_table& tb = tabs[t];
    pt_tsr_band b;
    memset(&b, 0, sizeof(b));
    b.full = 1; b.row1 = inp_h; b.keep1 = inp_h / kFrontStride; b.stack = -1;
    // the rows tsr_preprocess_kernel can write anything but the border value to: its own arithmetic for the source row (no column term: minv[3] == 0)
    int c0 = inp_h, c1 = -1;
    // no rotation / shear term: none the kernel's 10-bit fixed point can see anywhere on the map (the host's 3-point solve leaves terms of 1e-17)
    const bool axis = fabs(tb.minv[3]) * inp_w * 1024.0 < 0.5 && fabs(tb.minv[1]) * inp_h * 1024.0 < 0.5;
    const bool letterbox = inp_h % AL == 0 && tb.crop_h < tb.crop_w && axis && tb.minv[4] > 0.0;
    if (letterbox) {
      // source row of destination row y; it does not fall as y grows (minv[4] > 0: products, sums and roundings are all monotone)
      auto src_row = [&](int y) {
        const long long Y = (sat((tb.minv[4] * y + tb.minv[5]) * 1024.0) + 16) >> 5;
        const long long sy = Y >> 5;
        return sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
      };
      // a row has one of its two source rows (sy, sy + 1) in the crop when -1 <= sy < crop_h: the first row with sy >= -1, the first with sy >= crop_h
      auto first_at = [&](long long v) {
        int lo = 0, hi = inp_h;
        while (lo < hi) {
          const int mid = (lo + hi) / 2;
          if (src_row(mid) >= v) hi = mid;
          else lo = mid + 1;
        }
        return lo;
      };
      c0 = first_at(-1);
      c1 = first_at(tb.crop_h) - 1;
    }
    if (letterbox && c0 <= c1) {
      const int lo = c0 - kBandSlack - 2 * R, hi = c1 + 1 + kBandSlack + 2 * R;
      const int A = lo >= 0 ? lo / AL * AL : -AL, B = (hi + AL - 1) / AL * AL;
      // a window that meets the map's first or last AL rows runs the whole map: there the convolutions' zero padding is part of the result
      if (A >= AL && B <= inp_h - AL && B - A <= cap) {
        b.full = 0; b.row0 = A; b.row1 = B;
        // map row r (input row 4 r) sees input rows 4 r - R .. 4 r + R
        b.keep0 = (c0 - kBandSlack - R + kFrontStride - 1) / kFrontStride;
        b.keep1 = (c1 + kBandSlack + R) / kFrontStride + 1;
        if (stack < 0 || used + (B - A) > cap) { ++stack; used = 0; }
        b.stack = stack; b.stack_row = used;
        used += B - A;
      }
    }
    planned += b.row1 - b.row0;
    out[t] = b;
  }
  if (n_stacks) *n_stacks = stack + 1;
  if (row_fraction) *row_fraction = (double)planned / ((double)n * inp_h);
  return PT_OK;
}

int pt_launch_dcn_im2col(const bf16_t* x, const float* om, bf16_t* cols, int B, int H, int W, int C, int split,
                         hipStream_t s);
namespace {

struct Ctx : DlaCtx {
  struct UpTail {      // the next IDAUp step's `up(p) + this output`, run in a node DCN's epilogue (dcn_fused64_kernel's UPF): f = 0: none
    T p;
    const PtTensor* w = nullptr;
    int f = 0;
  };
  // DeformConv (lore_dla_34.py:65-83); up: out = up(up->p) + DeformConv(x)
  T dcn(const std::string& q, const T& x, int cout, const UpTail* up = nullptr) {
    T o = alloc(x.H, x.W, cout);
    static const bool fused = !(getenv("PT_DCN_FUSED") && atoi(getenv("PT_DCN_FUSED")) == 0);
    // the 27-channel offset / mask conv: inside the deformable conv's kernel where that kernel can (dcn_fused64_kernel<..., OMF = 1>: no launch, no fp32 map
    // through HBM), else as a launch of its own writing `om`
    const bool om_inside = fused && pt_dcn_fuses_om(e, x.C, x3);
    if (!om_inside) conv(x, q + ".om", 64, 3, 1, T(), 0, nullptr, 32, om, 32, 0, 27);     // 18 offsets + 9 masks are the layer's real outputs
    if (fused) {
      const PtTensor* w = get(q + (x3 ? ".dcn.w3" : ".dcn.w"));
      const PtTensor* b = get(q + ".dcn.b");
      const PtTensor* ow = om_inside ? get(q + (x3 ? ".om.w3" : ".om.w")) : nullptr;
      const PtTensor* ob = om_inside ? get(q + ".om.b") : nullptr;
      if (go()) {
        const int r = pt_launch_dcn_fused(e, x.p, om, W(w), F(b), o.p, n, x.H, x.W, x.C, cout, x3, 1, s, ow ? W(ow) : nullptr, ob ? F(ob) : nullptr,
                                          up ? up->p.p : nullptr, up ? F(up->w) : nullptr, up ? up->f : 0);
        if (r != PT_OK) rc = r;
      }
      return o;
    }
    // two-kernel form (PT_DCN_FUSED=0): columns through HBM, then a 1x1 GEMM
    if (go()) {
      PtProfScope ps(e, s, PT_PROF_OTHER, 0, "dcn im2col");
      const int r = pt_launch_dcn_im2col(x.p, om, cols, n, x.H, x.W, x.C, x3, s);
      if (r != PT_OK) rc = r;
    }
    T c;
    c.p = cols; c.H = x.H; c.W = x.W; c.C = 9 * x.C;
    conv(c, q + ".dcn", cout, 1, 1, o, 1);
    return o;
  }
  // IDAUp.forward (lore_dla_34.py:106-112) on layers[startp .. endp).
  // Where the node DCN can (pt_dcn_fuses_up), step j + 1's `up(proj) + node_j output` runs in node_j's epilogue: proj_{j+1} -- it reads layers[i + 1] only --
  // is issued before node_j, and the `dw convT up + add` launch remains for the first step alone, whose skip is somebody else's output.
  // A fused node never writes its own output, only the sum: `own_nodes` says that nobody but the next step reads the node outputs below the last --
  // true for ida_2 and ida_up; ida_0 / ida_1 leave theirs in `layers`, where the next IDAUp projects them (DLAUp.forward :128-134).
  // tail: what the LAST node adds in the same way (ida_2's last node forms ida_up's first sum); first_sum: that sum, received (the first step then
  // launches neither its proj nor its up-sampler: the caller has)
  void ida(const std::string& q, std::vector<T>& layers, int startp, int endp, int o_ch, const int* up_f, bool own_nodes = false,
           const UpTail* tail = nullptr, const T* first_sum = nullptr) {
    const bool fuse = own_nodes && pt_dcn_fuses_up(e, o_ch, o_ch, x3);
    T p, u;
    bool have_p = false, have_u = false;
    if (first_sum) { u = *first_sum; have_p = have_u = true; }
    for (int i = startp + 1; i < endp; ++i) {
      const int j = i - startp;
      const std::string js = std::to_string(j);
      if (!have_p) p = dcn(q + ".proj_" + js, layers[i], o_ch);
      if (!have_u) {
        const int f = up_f[j];
        u = alloc(p.H * f, p.W * f, o_ch);
        const PtTensor* wu = get(q + ".up_" + js + ".wf32");
        if (go()) {
          e->prof.next_bytes = (double)n * p.H * p.W * o_ch * 2.0 * mul * (1.0 + 2.0 * f * f);      // in once, skip + out at f x f the pixels
          char label[48];
          snprintf(label, sizeof(label), "dw convT up + add %d @%dx%d", o_ch, p.H * f, p.W * f);
          PtProfScope ps(e, s, PT_PROF_OTHER, 0, label);
          const int r = pt_launch_dwconvt_up_add(p.p, F(wu), layers[i - 1].p, u.p, n, p.H, p.W, o_ch, f, x3, s);
          if (r != PT_OK) rc = r;
        }
      }
      have_p = have_u = false;
      UpTail nx;
      if (fuse && i + 1 < endp) {
        const std::string ns = std::to_string(j + 1);
        p = nx.p = dcn(q + ".proj_" + ns, layers[i + 1], o_ch);
        nx.w = get(q + ".up_" + ns + ".wf32");
        nx.f = up_f[j + 1];
        have_p = true;
      } else if (fuse && tail) {
        nx = *tail;
      }
      layers[i] = dcn(q + ".node_" + js, u, o_ch, nx.f ? &nx : nullptr);
      if (nx.f) { u = layers[i]; have_u = true; }      // the next step's sum, already
    }
  }
};

}  // namespace

// x: NHWC4 bf16 [n, H, W, 4] ([hi rgb0 | lo rgb0] in BF16X3 mode); heads: fp32 NHWC at H/4 x W/4 with channel
// strides 8 (hm: 2 valid), 8 (st), 8 (wh), 256 (ax), 256 (cr), 8 (reg: 2 valid)
struct BandArgs {        // warp inside the call (pt_lore_warp_forward_decode): the tables on both sides, the pages they are cut from
  const uint8_t* pages;
  int ph, pw;
  const pt_tsr_table *h_tabs, *d_tabs;
  int bgr, bands, margin;
  bf16_t* l2_out;        // test hook: stop behind level 2
};

// [3][256] ((v / 255.) - mean) / std in float64 then cast, as numpy evaluates processer_lore.py:67-70,90
int pt_lore_norm_lut(pt_engine* e, const float** lut_out) {
  if (!e->tsr_lut) {
    const float mean[3] = {0.408f, 0.447f, 0.470f}, stdv[3] = {0.289f, 0.274f, 0.278f};
    float lut[768];
    for (int c = 0; c < 3; ++c)
      for (int v = 0; v < 256; ++v) lut[c * 256 + v] = (float)(((double)v / 255.0 - (double)mean[c]) / (double)stdv[c]);
    PT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->tsr_lut), sizeof(lut)));
    PT_HIP_CHECK(hipMemcpy(e->tsr_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
  }
  *lut_out = e->tsr_lut;
  return PT_OK;
}

// host array -> device (arena) behind the launches queued so far, through the engine's pinned ring of band tables
static int upload_small(pt_engine* e, void* d_dst, const void* h_src, size_t bytes, hipStream_t s) {
  void* hs = e->band_ring.acquire(bytes);
  PT_REQUIRE(hs, "Lore net: pinned staging allocation failed");
  memcpy(hs, h_src, bytes);
  PT_HIP_CHECK(hipMemcpyAsync(d_dst, hs, bytes, hipMemcpyHostToDevice, s));
  PT_REQUIRE(e->band_ring.release(s) == 0, "Lore net: event record failed");
  return PT_OK;
}

// The front segment with the letterbox rows left out: warp the planned rows (whole maps of the `full` tables, then the bands, stacked into tall
// one-image inputs), run base_layer .. level2 on the full group and on every stack, and assemble `layers[2]` of all n tables from the bands' kept rows
// and the cached map of an all-padding table.  `in`: [n * H, W, 4 | 8] from the arena.  Returns the assembled map in layers[2].
static int lore_band_front(Ctx& c, std::vector<T>& layers, const BandArgs& bd, const std::vector<pt_tsr_band>& plan, int n_stacks, const float* lut,
                           bf16_t* in, int H, int W) {
  pt_engine* e = c.e;
  hipStream_t s = c.s;
  const int n = c.n, px = 4 * c.mul, AL = PT_TSR_BAND_ALIGN, rows4 = H / kFrontStride, row_elems = W / kFrontStride * 64 * c.mul;
  // where everything lies in `in`: the full tables' maps first, then the stacks
  std::vector<int> stack_rows(n_stacks, 0), stack_off(n_stacks, 0), full_idx(n, -1);
  int nf = 0;
  for (int t = 0; t < n; ++t) {
    if (plan[t].full) full_idx[t] = nf++;
    else stack_rows[plan[t].stack] += plan[t].row1 - plan[t].row0;
  }
  for (int k = 0, off = nf * H; k < n_stacks; off += stack_rows[k], ++k) stack_off[k] = off;
  const int runs_max = n * ((H + AL - 1) / AL);      // the all-full case: device tables and arena use do not depend on the plan
  int4* d_runs = c.take<int4>((size_t)runs_max * sizeof(int4));
  PtBandSrc* d_src = c.take<PtBandSrc>((size_t)n * sizeof(PtBandSrc));
  T l2 = c.alloc(rows4, W / kFrontStride, 64);
  const size_t o1 = c.mark();
  {      // what the segment takes when every table runs in full: the arena is sized for that
    const bool dry = c.dry;
    c.dry = true;
    std::vector<T> tmp(6);
    dla34_front(c, tmp, in, H, W);
    c.dry = dry;
  }
  const size_t worst = c.mark() + (64u << 10);      // (+ the alignment gaps of the few more takes several groups make)
  c.rewind(o1);
  if (c.go()) {
    std::vector<int4> runs;
    runs.reserve(runs_max);
    for (int t = 0; t < n; ++t) {
      const pt_tsr_band& b = plan[t];
      const int dst = b.full ? full_idx[t] * H : stack_off[b.stack] + b.stack_row;
      for (int y = b.row0; y < b.row1; y += AL) runs.push_back(int4{t, y, dst + (y - b.row0), 0});
    }
    PT_REQUIRE((int)runs.size() <= runs_max, "Lore net: band plan larger than the batch");
    int r = upload_small(e, d_runs, runs.data(), runs.size() * sizeof(int4), s);
    if (r == PT_OK) r = pt_launch_tsr_preprocess_rows(e, bd.pages, bd.ph, bd.pw, bd.d_tabs, d_runs, (int)runs.size(), H, W, bd.bgr, lut, in, c.x3, s);
    if (r != PT_OK) return r;
  }
  // every group chooses its kernels as the whole batch does
  c.pick_n = n; c.whole_H = H;
  // the all-padding table's level-2 map: once per (weights, precision, input size, kernel family of the 64 -> 64 layers)
  const int pi = e->precision & 3;
  const int key[3] = {H, W, (!c.x3 && pt_conv_takes_ws64(e, n, rows4, W / kFrontStride)) ? 1 : 0};
  const size_t pad_bytes = (size_t)rows4 * row_elems * sizeof(bf16_t);
  if (!e->tsr_pad_l2_valid[pi] || memcmp(e->tsr_pad_l2_key[pi], key, sizeof(key)) != 0) {
    c.n = 1; c.part_H = H;
    bf16_t* pin = c.take<bf16_t>((size_t)H * W * px * sizeof(bf16_t));
    if (c.go()) {
      if (e->tsr_pad_l2_cap[pi] < pad_bytes) {
        if (e->tsr_pad_l2[pi]) PT_HIP_CHECK(hipFree(e->tsr_pad_l2[pi]));      // (waits for the device: nobody reads the old block any more)
        e->tsr_pad_l2[pi] = nullptr; e->tsr_pad_l2_cap[pi] = 0;
        PT_HIP_CHECK(hipMalloc(&e->tsr_pad_l2[pi], pad_bytes));
        e->tsr_pad_l2_cap[pi] = pad_bytes;
      }
      const int r = pt_launch_tsr_pad_image(lut, H, W, pin, c.x3, s);
      if (r != PT_OK) return r;
    }
    std::vector<T> pl(6);
    dla34_front(c, pl, pin, H, W);
    if (c.go()) {
      PT_HIP_CHECK(hipMemcpyAsync(e->tsr_pad_l2[pi], pl[2].p, pad_bytes, hipMemcpyDeviceToDevice, s));
      e->tsr_pad_l2_valid[pi] = true;
      memcpy(e->tsr_pad_l2_key[pi], key, sizeof(key));
      // later calls may run on another stream: they wait for this build through the event
      if (!e->tsr_pad_l2_ready[pi]) PT_HIP_CHECK(hipEventCreateWithFlags(&e->tsr_pad_l2_ready[pi], hipEventDisableTiming));
      PT_HIP_CHECK(hipEventRecord(e->tsr_pad_l2_ready[pi], s));
    }
    c.n = n;
    c.rewind(o1);
  } else if (c.go() && e->tsr_pad_l2_ready[pi]) {
    PT_HIP_CHECK(hipStreamWaitEvent(s, e->tsr_pad_l2_ready[pi], 0));      // a no-op once the build has completed
  }
  T full_l2;
  std::vector<T> stack_l2(n_stacks);
  if (nf) {
    c.n = nf; c.part_H = H;
    std::vector<T> fl(6);
    dla34_front(c, fl, in, H, W);
    full_l2 = fl[2];
  }
  for (int k = 0; k < n_stacks; ++k) {
    c.n = 1; c.part_H = stack_rows[k];
    std::vector<T> sl(6);
    dla34_front(c, sl, in + (size_t)stack_off[k] * W * px, stack_rows[k], W);
    stack_l2[k] = sl[2];
  }
  c.n = n; c.pick_n = 0;
  if (c.go()) {
    std::vector<PtBandSrc> src(n);
    for (int t = 0; t < n; ++t) {
      const pt_tsr_band& b = plan[t];
      if (b.full) src[t] = PtBandSrc{(full_l2.p - l2.p) + (long long)full_idx[t] * rows4 * row_elems, 0, 0, rows4, 0};
      else src[t] = PtBandSrc{(stack_l2[b.stack].p - l2.p) + (long long)(b.stack_row / kFrontStride) * row_elems, b.row0 / kFrontStride, b.keep0, b.keep1, 0};
    }
    int r = upload_small(e, d_src, src.data(), src.size() * sizeof(PtBandSrc), s);
    if (r == PT_OK) r = pt_launch_tsr_band_assemble(e, d_src, reinterpret_cast<const bf16_t*>(e->tsr_pad_l2[pi]), l2.p, n, rows4, row_elems, s);
    if (r != PT_OK) return r;
  }
  c.reserve_to(worst);
  layers[2] = l2;
  return PT_OK;
}

struct SparseArgs {      // fused forward + decode: the ax / cr heads run on patch mosaics around the decoded positions
  int wiz_rev;
  float vis_thresh;
  int* d_counts;
  float *d_dets, *d_logi;
};

static int lore_dla_run(pt_engine* e, const bf16_t* x, int n, int H, int W, float* hm, float* st, float* wh, float* ax,
                        float* cr, float* reg, const SparseArgs* sp, hipStream_t s, const BandArgs* bd = nullptr) {
  PT_REQUIRE(H % 32 == 0 && W % 32 == 0 && H > 0 && W > 0, "Lore net: input %dx%d must be multiples of 32", H, W);
  PT_REQUIRE((x || bd) && n > 0 && (sp || (bd && bd->l2_out) || (hm && st && wh && ax && cr && reg)), "Lore net: null pointer");
  const PtModel* m = pt_find_model(e, PT_MODEL_LORE_DLA34, "Lore DLA-34", "PT_MODEL_LORE_DLA34");
  if (!m) return PT_ERR_STATE;
  // warp inside the call: the row bands the front segment needs, planned on the host
  const float* lut = nullptr;
  std::vector<pt_tsr_band> plan;
  int n_stacks = 0, n_banded = 0;
  if (bd) {
    const int r = pt_lore_norm_lut(e, &lut);
    if (r != PT_OK) return r;
  }
  if (bd && bd->bands) {
    const char* cap_env = getenv("PT_TSR_BAND_STACK_ROWS");      // tests: a low cap splits a batch into several stacks (read per call)
    int cap = kBandStackCap / (pt_split(e) ? 2 : 1);             // the pair modes' maps are twice the bytes
    if (cap_env && atoi(cap_env) > 0 && atoi(cap_env) < cap) cap = atoi(cap_env);
    plan.resize(n);
    const int r = pt_lore_plan_bands(bd->h_tabs, n, H, W, cap, bd->margin, plan.data(), &n_stacks, nullptr);
    if (r != PT_OK) return r;
    for (int t = 0; t < n; ++t) n_banded += plan[t].full ? 0 : 1;
  }
  Ctx c;
  c.init(e, m, "Lore DLA-34", s, n, PT_ARENA_TSR);
  float* heads[6] = {hm, st, wh, ax, cr, reg};
  const char* hname[6] = {"hm", "st", "wh", "ax", "cr", "reg"};
  const int hcs[6] = {8, 8, 8, 256, 256, 8};
  const int hreal[6] = {2, 8, 8, 256, 256, 2};     // the heads' real channel counts (roofline accounting)

  return pt_plan_then_launch(c, "Lore net", [&]() -> int {
    // shared DCN scratch: the largest site is 64 channels at H/4 x W/4 (9*64 columns); 128 ch at H/8 is half of it
    const size_t px4 = (size_t)n * (H / 4) * (W / 4);
    c.cols = c.take<bf16_t>(px4 * 576 * c.mul * sizeof(bf16_t));
    c.om = c.take<float>(px4 * 32 * sizeof(float));

    std::vector<T> layers(6);
    if (!bd) {
      dla34_front(c, layers, x, H, W);
    } else {
      bf16_t* in = c.take<bf16_t>((size_t)n * H * W * 4 * c.mul * sizeof(bf16_t));
      if (n_banded) {
        const int r = lore_band_front(c, layers, *bd, plan, n_stacks, lut, in, H, W);
        if (r != PT_OK) return r;
      } else {      // nothing to skip (or PT_TSR_BANDS off in the hook): the warp and the segment on whole maps
        if (c.go()) {
          const int r = pt_launch_tsr_preprocess(bd->pages, bd->ph, bd->pw, bd->d_tabs, n, H, W, bd->bgr, lut, in, c.x3, s);
          if (r != PT_OK) return r;
        }
        dla34_front(c, layers, in, H, W);
      }
      if (bd->l2_out) {
        if (c.go()) PT_HIP_CHECK(hipMemcpyAsync(bd->l2_out, layers[2].p, (size_t)n * (H / 4) * (W / 4) * 64 * c.mul * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
        return c.rc;
      }
    }
    dla34_rest(c, layers);

    // DLAUp.forward (lore_dla_34.py:128-134): ida_0 on [4,6), ida_1 on [3,6), ida_2 on [2,6)
    std::vector<T> out = {layers[5]};
    const int f2[4] = {1, 2, 2, 2};
    c.ida("dla_up.ida_0", layers, 4, 6, 256, f2);
    out.insert(out.begin(), layers[5]);
    c.ida("dla_up.ida_1", layers, 3, 6, 128, f2);
    out.insert(out.begin(), layers[5]);
    // ida_up's first sum up_1(proj_1(out[1])) + out[0] has ida_2's last node as its skip: proj_1 reads ida_1's result, so it can run before ida_2,
    // whose last node then adds its up-sampled map in the epilogue
    const int f24[3] = {1, 2, 4};
    Ctx::UpTail t2;
    if (pt_dcn_fuses_up(e, 64, 64, c.x3)) {
      t2.p = c.dcn("ida_up.proj_1", out[0], 64);
      t2.w = c.get("ida_up.up_1.wf32");
      t2.f = f24[1];
    }
    c.ida("dla_up.ida_2", layers, 2, 6, 64, f2, true, t2.f ? &t2 : nullptr);
    out.insert(out.begin(), layers[5]);
    // ida_up on clones of out[0..3) (strides 4, 8, 16): up factors 2 and 4
    std::vector<T> y = {out[0], out[1], out[2]};
    c.ida("ida_up", y, 0, 3, 64, f24, true, nullptr, t2.f ? &y[0] : nullptr);
    const T feat = y[2];
    // hm.0 + hm.2 in one launch (conv3x3_pipe_persist_hm_kernel): the 256-channel hidden map is never stored; PT_LORE_HM_FUSE=0: the two launches
    const bool hm_fused = pt_conv_fuses_hm(e);
    // sparse: with the fused head nobody needs `hid`, nor the logit map -- the launch writes the scores where the peak test reads them
    T hid;
    if (!(sp && hm_fused)) hid = c.alloc(feat.H, feat.W, 256);
    // only `hm` is needed everywhere: the other five heads run on patch mosaics (lore_decode.hip)
    if (sp && !hm_fused) heads[0] = c.take<float>((size_t)n * feat.H * feat.W * 8 * sizeof(float));
    for (int h = 0; h < 6; ++h) {
      if (sp && h != 0) continue;
      if (h == 0 && hm_fused) {
        const PtTensor* w2 = c.get("hm.2.w");
        const PtTensor* b2 = c.get("hm.2.b");
        ConvDesc d;
        if (!c.conv_desc(d, feat, "hm.0", 256, 3, 1, 1)) continue;
        d.hm_w2 = c.W(w2); d.hm_b2 = c.F(b2);
        if (sp) {
          const int r = pt_lore_decode_sig_map(e, n, feat.H, feat.W, &d.hm_sig);
          if (r != PT_OK) return r;
        } else {
          d.hm_logits = heads[0];
        }
        c.launch(d);
        continue;
      }
      c.conv(feat, std::string(hname[h]) + ".0", 256, 3, 1, hid, 1);
      c.conv(hid, std::string(hname[h]) + ".2", hcs[h] < 64 ? 64 : hcs[h], 1, 1, T(), 0, nullptr, hcs[h], heads[h], hcs[h], 0, hreal[h]);
    }
    if (sp) {
      int rows_ax = 0, rows_cr = 0, rows_cell = 0, rows_corner = 0;
      pt_lore_mosaic_rows(n, &rows_ax, &rows_cr, &rows_cell, &rows_corner);
      const int MW = 32;          // patches per row of the patch image (lore_decode.hip: MOS_PW); a patch = one row of 9 * 64 values
      auto mosaic = [&](int rows, int C) {
        T t;
        t.H = rows; t.W = MW; t.C = C;
        t.p = c.take<bf16_t>(((size_t)rows * MW * C * c.mul + 64) * sizeof(bf16_t));
        return t;
      };
      T mcell = mosaic(rows_cell, 9 * 64), mcorner = mosaic(rows_corner, 9 * 64), max_ = mosaic(rows_ax, 9 * 64), mcr_ = mosaic(rows_cr, 9 * 64);
      T mhid = mosaic(rows_cr, 256);                 // hidden layer of whichever head is running (rows_cr is the largest)
      float* o_wh = c.take<float>((size_t)rows_cell * MW * 8 * sizeof(float));
      float* o_regc = c.take<float>((size_t)rows_cell * MW * 8 * sizeof(float));
      float* o_st = c.take<float>((size_t)rows_corner * MW * 8 * sizeof(float));
      float* o_regk = c.take<float>((size_t)rows_corner * MW * 8 * sizeof(float));
      float* oax = c.take<float>((size_t)rows_ax * MW * 256 * sizeof(float));
      float* ocr = c.take<float>((size_t)rows_cr * MW * 256 * sizeof(float));
      if (c.go()) {
        const int keep = c.n;
        // one head on one mosaic: 3x3 (64 -> 256) + ReLU, then 1x1 to nc channels, fp32 out; tiles below `lim` rows exit
        auto head = [&](const T& mos, int rows, const char* name, int nc, float* outp, const int* lim, int real_nc) {
          T hh = mhid;
          hh.H = rows;
          c.n = 1;
          c.ylimit = lim;
          // the 3x3 layer as a GEMM over patch rows: K = 9 * 64 in the conv kernel's own (chunk, tap, channel) order, so the
          // layer's packed 3x3 weight tiles are the 18 K-chunks of this 1x1 launch as they stand
          c.conv(mos, std::string(name) + ".0", 256, 1, 1, hh, 1);
          c.conv(hh, std::string(name) + ".2", nc < 64 ? 64 : nc, 1, 1, T(), 0, nullptr, nc, outp, nc, 0, real_nc);
          c.ylimit = nullptr;
          c.n = keep;
        };
        const int *lim_cell = nullptr, *lim_corner = nullptr, *lim_ax = nullptr, *lim_cr = nullptr;
        int r = pt_lore_decode_peaks(e, heads[0], n, feat.H, feat.W, sp->wiz_rev, sp->vis_thresh, sp->d_counts, &lim_cell,
                                     &lim_corner, s);
        if (r == PT_OK) r = pt_lore_peak_patches(e, feat.p, n, feat.H, feat.W, 64, c.x3, mcell.p, mcorner.p, s);
        if (r != PT_OK) return r;
        head(mcell, rows_cell, "wh", 8, o_wh, lim_cell, 8);
        head(mcell, rows_cell, "reg", 8, o_regc, lim_cell, 2);
        head(mcorner, rows_corner, "st", 8, o_st, lim_corner, 8);
        head(mcorner, rows_corner, "reg", 8, o_regk, lim_corner, 2);
        if (c.rc != PT_OK) return c.rc;
        r = pt_lore_decode_boxes(e, o_regc, o_wh, o_regk, o_st, n, feat.H, feat.W, &lim_ax, &lim_cr, s);
        if (r == PT_OK) r = pt_lore_patch_gather(e, feat.p, n, feat.H, feat.W, 64, c.x3, max_.p, mcr_.p, s);
        if (r != PT_OK) return r;
        head(max_, rows_ax, "ax", 256, oax, lim_ax, 256);
        head(mcr_, rows_cr, "cr", 256, ocr, lim_cr, 256);
        if (c.rc != PT_OK) return c.rc;
        r = pt_lore_decode_sparse(e, oax, ocr, n, feat.H, feat.W, sp->vis_thresh, sp->d_counts, sp->d_dets, sp->d_logi, s);
        if (r != PT_OK) return r;
      }
    }
    return c.rc;
  });
}


int pt_lore_forward_net(pt_engine* e, const bf16_t* x, int n, int H, int W, float* hm, float* st, float* wh, float* ax,
                        float* cr, float* reg, hipStream_t s) {
  PT_REQUIRE(hm && st && wh && ax && cr && reg, "Lore net: null pointer");
  return lore_dla_run(e, x, n, H, W, hm, st, wh, ax, cr, reg, nullptr, s);
}

// DLA-34 forward and decode in one call with sparse ax / cr heads (see lore_decode.hip); outputs as pt_lore_decode
int pt_lore_forward_decode(pt_engine* e, const bf16_t* x, int n, int H, int W, int wiz_rev, float vis_thresh, int* d_counts,
                           float* d_dets, float* d_logi, hipStream_t s) {
  PT_REQUIRE(d_counts && d_dets && d_logi, "Lore forward+decode: null pointer");
  SparseArgs sp{wiz_rev, vis_thresh, d_counts, d_dets, d_logi};
  return lore_dla_run(e, x, n, H, W, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &sp, s);
}

// warp + forward + decode with the tables known on the host: the front segment skips the letterbox rows (lore_band_front)
int pt_lore_warp_forward_decode(pt_engine* e, const uint8_t* pages, int ph, int pw, const pt_tsr_table* h_tabs, const pt_tsr_table* d_tabs, int n, int H,
                                int W, int bgr, int bands, int margin, int wiz_rev, float vis_thresh, int* d_counts, float* d_dets, float* d_logi,
                                bf16_t* l2_out, hipStream_t s) {
  PT_REQUIRE(pages && h_tabs && d_tabs && ph > 0 && pw > 0 && (l2_out || (d_counts && d_dets && d_logi)), "Lore warp+forward+decode: null pointer");
  SparseArgs sp{wiz_rev, vis_thresh, d_counts, d_dets, d_logi};
  BandArgs bd{pages, ph, pw, h_tabs, d_tabs, bgr, bands, margin, l2_out};
  return lore_dla_run(e, nullptr, n, H, W, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, l2_out ? nullptr : &sp, s, &bd);
}

// ---------------------------------------------------------------------------------------------------------------------
// 'wireless' detector: LoreDetectModel.forward (lore/lore_detector.py:353-389) -- ResNet-18-style backbone whose every
// stage is strided, four ConvTranspose2d(4x4, stride 2) + BN + ReLU up-samplers (run as 3x3 convolutions with 4 x 256
// outputs and a pixel-shuffle epilogue), 1x1 lateral `adaption` convs added through the residual path, heads of
// four 3x3 (-> 64) + ReLU and a 1x1.  Same head-map outputs as pt_lore_forward_net.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct WCtx : NetCtx {
  void conv(const T& in, const std::string& q, int N, int ks, int stride, const T& out, int relu, const T* res = nullptr,
            int shuffle = 0, int nv = 0, float* out_f32 = nullptr, int f32_cs = 0) {
    ConvDesc c;
    if (!conv_desc(c, in, q, N, ks, stride, relu)) return;
    c.n_valid = nv; c.shuffle_cout = shuffle;
    if (shuffle && ks == 3) c.alg_scale = 16.0 / 36.0;   // ConvTranspose2d(k=4,s=2) has 16 taps per (input pixel, Cout); the 3x3 x 4-phase GEMM spends 36
    if (out_f32) to_f32(c, out_f32, f32_cs);
    else to_map(c, out);
    if (res) { c.res = res->p; c.res_mode = 1; }
    launch(c);
  }
};

}  // namespace

int pt_lore_wireless_forward_net(pt_engine* e, const bf16_t* x, int n, int H, int W, float* hm, float* st, float* wh,
                                 float* ax, float* cr, float* reg, hipStream_t s) {
  PT_REQUIRE(H % 64 == 0 && W % 64 == 0 && H > 0 && W > 0, "Lore wireless net: input %dx%d must be multiples of 64", H, W);
  PT_REQUIRE(x && hm && st && wh && ax && cr && reg && n > 0, "Lore wireless net: null pointer");
  const PtModel* m = pt_find_model(e, PT_MODEL_LORE_RESNET18, "Lore wireless", "PT_MODEL_LORE_RESNET18");
  if (!m) return PT_ERR_STATE;
  WCtx c;
  c.init(e, m, "Lore wireless", s, n, PT_ARENA_TSR);
  float* heads[6] = {hm, st, wh, ax, cr, reg};
  const char* hname[6] = {"hm", "st", "wh", "ax", "cr", "reg"};
  const int hcs[6] = {8, 8, 8, 256, 256, 8};
  const int planes[4] = {64, 128, 256, 256};
  return pt_plan_then_launch(c, "Lore wireless net", [&] {
    T s0 = c.alloc(H / 2, W / 2, 64);
    const PtTensor* w = c.get(c.x3 ? "stem.w3" : "stem.w");
    const PtTensor* b = c.get("stem.b");
    if (c.go()) {
      const int r = pt_launch_stem7x7(e, x, n, H, W, c.W(w), c.F(b), s0.p, c.x3, s, 2, 0);
      if (r != PT_OK) c.rc = r;
    }
    T x0 = c.alloc(H / 4, W / 4, 64);
    if (c.go()) {
      PtProfScope ps(e, s, PT_PROF_OTHER, 0, "maxpool");
      const int r = pt_launch_maxpool3x3s2(s0.p, n, H / 2, W / 2, 64, x0.p, c.x3, s);
      if (r != PT_OK) c.rc = r;
    }
    T feat[4];
    T cur = x0;
    for (int l = 0; l < 4; ++l) {
      for (int b = 0; b < 2; ++b) {
        const std::string q = "layer" + std::to_string(l + 1) + "." + std::to_string(b);
        const int stride = b == 0 ? 2 : 1;
        T t = c.alloc(cur.H / stride, cur.W / stride, planes[l]);
        c.conv(cur, q + ".conv1", planes[l], 3, stride, t, 1);
        T res = cur;
        if (b == 0) {
          res = c.alloc(t.H, t.W, planes[l]);
          c.conv(cur, q + ".down", planes[l], 1, 2, res, 0);
        }
        T o = c.alloc(t.H, t.W, planes[l]);
        c.conv(t, q + ".conv2", planes[l], 3, 1, o, 1, &res);
        cur = o;
      }
      feat[l] = cur;
    }
    // top-down: deconv (3x3 + pixel shuffle + BN + ReLU), then `adaption(lateral) + deconv`
    T up = feat[3];
    const T* lateral[4] = {&feat[2], &feat[1], &feat[0], &x0};
    const char* adapt[4] = {"adaption3", "adaption2", "adaption1", "adaption0"};
    for (int i = 0; i < 4; ++i) {
      T d = c.alloc(up.H * 2, up.W * 2, 256);
      c.conv(up, "deconv" + std::to_string(i + 1), 1024, 3, 1, d, 1, nullptr, 256);
      T o = c.alloc(d.H, d.W, 256);
      c.conv(*lateral[i], adapt[i], 256, 1, 1, o, 0, &d);
      up = o;
    }
    T f = c.alloc(up.H, up.W, 256);
    c.conv(up, "adaptionU1", 256, 1, 1, f, 0);
    T h1 = c.alloc(f.H, f.W, 64), h2 = c.alloc(f.H, f.W, 64);
    for (int h = 0; h < 6; ++h) {
      const int n3 = h == 5 ? 1 : 4;
      const T* in = &f;
      for (int j = 0; j < n3; ++j) {
        const T& o = (j & 1) ? h2 : h1;
        c.conv(*in, std::string(hname[h]) + ".c" + std::to_string(j), 64, 3, 1, o, 1);
        in = &o;
      }
      c.conv(*in, std::string(hname[h]) + ".out", hcs[h] < 64 ? 64 : hcs[h], 1, 1, T(), 0, nullptr, 0, hcs[h], heads[h], hcs[h]);
    }
    return c.rc;
  });
}

}  // namespace PT_FMT_NS
