// net_ctx.h -- the host-side plumbing every model graph shares: the map descriptor, the weight-blob lookup, the launch context
// (arena accounting, tensor fetch, ConvDesc builder, rc latch) and the one place an activation arena is planned, grown and
// re-planned.  Included by one translation unit per model; everything here is internal to it.
#pragma once

#include <stdio.h>

#include <string>

#include "common.h"

namespace PT_FMT_NS {

namespace {

struct T {      // an NHWC activation map in an arena ((hi | lo) channel groups in the pair modes)
  bf16_t* p = nullptr;
  int H = 0, W = 0, C = 0;
};

inline const float* F(const PtTensor* t) { return reinterpret_cast<const float*>(t->d_ptr); }
inline const bf16_t* W(const PtTensor* t) { return reinterpret_cast<const bf16_t*>(t->d_ptr); }

// bf16 rows [rows, C] (rows a multiple of 32) as the one-image map [rows / 32, 32, C] a 1x1 GEMM reads
inline T rows_map(const bf16_t* x, long long rows, int C) { return T{const_cast<bf16_t*>(x), (int)(rows / 32), 32, C}; }

// the loaded blob of model `kind`, or null with the error set (PT_ERR_STATE either way: not loaded, or packed for the other
// storage format).  slot >= 0: one of several blobs of a kind, named "<enum_name> + <slot>" in the message
inline const PtModel* pt_find_model(pt_engine* e, int kind, const char* name, const char* enum_name, int slot = -1) {
  auto it = e->models.find(kind);
  if (it == e->models.end()) {
    char plus[16] = "";
    if (slot >= 0) snprintf(plus, sizeof(plus), " + %d", slot);
    pt_set_error("%s weights not loaded (pt_weights_load(%s%s))", name, enum_name, plus);
    return nullptr;
  }
  return pt_model_format_ok(it->second, enum_name) ? &it->second : nullptr;
}

// re-allocate an arena at its high-water mark (a plan that did not fit has just recorded it); the device is idle first, so no
// launch in flight still reads the old block
inline int pt_arena_grow(pt_engine* e, int arena) {
  PtArena& A = e->arenas[arena];
  PT_HIP_CHECK(hipDeviceSynchronize());
  if (A.base) PT_HIP_CHECK(hipFree(A.base));
  A.base = nullptr;
  A.cap = 0;
  const size_t want = pt_arena_round(A.high);
  PT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&A.base), want));
  A.cap = want;
  return PT_OK;
}

// launch context of one net forward: what the graph bodies allocate from, fetch weights through and launch on
struct NetCtx {
  pt_engine* e = nullptr;
  const PtModel* m = nullptr;
  const char* what = "";      // the model named in a missing-tensor error
  hipStream_t s = nullptr;
  int n = 1, x3 = 0, mul = 1;
  bool dry = false;           // planning pass: only arena accounting, no launches
  bool ok = true;             // arena had room for everything so far
  int rc = PT_OK;             // first error of a fetch or a launch; later launches are skipped
  int arena = 0;

  void init(pt_engine* e_, const PtModel* m_, const char* what_, hipStream_t s_, int n_, int arena_) {
    e = e_; m = m_; what = what_; s = s_; n = n_; arena = arena_;
    x3 = pt_split(e) ? 1 : 0;
    mul = x3 ? 2 : 1;
    dry = false; ok = true; rc = PT_OK;
  }
  template <class U>
  U* take(size_t bytes) {
    U* p = reinterpret_cast<U*>(e->arenas[arena].take(bytes));
    if (!p) ok = false;
    return p;
  }
  // a stretch of the arena used twice: mark(), takes, rewind(mark); reserve_to(off): the arena counts as used up to `off` (a worst case planned for,
  // whatever this call took), so that its high-water mark does not depend on the call's data
  size_t mark() const { return e->arenas[arena].off; }
  void rewind(size_t off) { e->arenas[arena].off = off; }
  void reserve_to(size_t off) {
    PtArena& A = e->arenas[arena];
    if (off <= A.off) return;
    if (off > A.cap) ok = false;
    A.off = off;
    if (off > A.high) A.high = off;
  }
  T alloc(int H, int W, int C) {
    T t;
    t.H = H; t.W = W; t.C = C;
    t.p = take<bf16_t>((size_t)n * H * W * C * mul * sizeof(bf16_t));
    return t;
  }
  const PtTensor* get(const std::string& name) {
    const PtTensor* t = m->find(name);
    if (!t && rc == PT_OK) {
      pt_set_error("%s weight blob lacks tensor '%s'", what, name.c_str());
      rc = PT_ERR_FORMAT;
    }
    return t;
  }
  bool go() const { return rc == PT_OK && !dry && ok; }
  // the casts as members too: c.W(t) reads well in a graph body, and works where an `int W` parameter hides the free function
  static const float* F(const PtTensor* t) { return PT_FMT_NS::F(t); }
  static const bf16_t* W(const PtTensor* t) { return PT_FMT_NS::W(t); }

  // conv / GEMM with folded bias over map `in`; q = weight name prefix.  false: nothing to launch (planning pass, or an error is latched)
  bool conv_desc(ConvDesc& c, const T& in, const std::string& q, int N, int ks, int stride, int act) {
    const PtTensor* w = get(q + (x3 ? ".w3" : ".w"));
    const PtTensor* b = get(q + ".b");
    if (!go()) return false;
    c.in = in.p; c.B = n; c.H = in.H; c.W = in.W; c.Cin = in.C;
    c.w = W(w); c.bias = F(b);
    c.N = N; c.ks = ks; c.stride = stride; c.relu = act; c.split = x3;
    return true;
  }
  void to_map(ConvDesc& c, const T& out) const { c.out = out.p; c.out_cstride = out.C * mul; c.out_lo_off = out.C; }
  void to_f32(ConvDesc& c, float* p, int cstride) const { c.out_f32 = p; c.out_cstride = cstride; }
  void launch(const ConvDesc& c) {
    const int r = pt_launch_conv(e, c, s);
    if (r != PT_OK) rc = r;
  }
};

// Run `body` (the whole graph: arena takes, weight fetches, launches guarded by c.go()) twice: pass 0 plans the arena and grows
// it if the plan did not fit, pass 1 launches.  body() -> PT_OK or an error, which ends the call at once.
template <class Body>
int pt_plan_then_launch(NetCtx& c, const char* label, Body&& body) {
  for (int pass = 0; pass < 2; ++pass) {
    c.dry = pass == 0;
    c.ok = true;
    c.e->arenas[c.arena].reset();
    int rc = body();
    if (rc != PT_OK) return rc;
    if (c.ok) continue;
    if (pass == 1) {
      pt_set_error("%s: activation arena allocation failed", label);
      return PT_ERR_HIP;
    }
    if ((rc = pt_arena_grow(c.e, c.arena)) != PT_OK) return rc;
  }
  return PT_OK;
}

// The nets that carve named buffers up front and then launch unconditionally: plan(take) performs the takes
// (take(bytes) -> void*, null while the arena is too small); it runs again after the arena has grown, so it assigns every pointer each time
template <class Plan>
int pt_arena_plan(pt_engine* e, int arena, const char* label, Plan&& plan) {
  NetCtx c;
  c.e = e; c.arena = arena;
  return pt_plan_then_launch(c, label, [&] {
    plan([&](size_t bytes) { return c.take<void>(bytes); });
    return PT_OK;
  });
}

}  // namespace

}  // namespace PT_FMT_NS
