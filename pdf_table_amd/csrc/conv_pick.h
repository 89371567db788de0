// conv_pick.h -- which kernel a dense convolution layer takes, as a pure host function.
//
// Plain C++17: nothing from HIP, nothing from common.h.  conv_igemm.hip's pt_launch_conv() describes the layer as a ConvShape, reads the
// environment into a ConvSwitches, asks conv_pick() and launches the instance it names; tools/conv_pick.cpp asks the same question without a GPU.
// Everything that decides is here once: the switches and how they are parsed, the selection rules in their order of precedence with the
// measurements behind them, the tile grid of a pick, its profile label and its kernel name.  The kernels, their tile constants and the
// runtime -> template table stay in conv_igemm.hip (which static_asserts that the tile sizes written here are the kernels' own).
#pragma once

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

// ---- switches ---------------------------------------------------------------------------------------------------------------------------
// Every environment switch of the dense-conv dispatch, each parsed once into an int with atoi (decimal integers; "abc" and "" are 0, "01" is 1).
// INTEGRATION.md section 5 has the table of what the other value of each runs.
struct ConvSwitches {
  static constexpr int kUnset = INT_MIN;
  // read once per process (A/B switches of a whole run)
  int conv1_direct = 1;      // PT_CONV1_DIRECT   0: the staged epilogue for every launch of the chunk kernel
  int conv_dma = 1;          // PT_CONV_DMA       0: no DMA-fed kernel at all (chunk / wide1 kernels everywhere)
  int conv_variant = 3;      // PT_CONV_VARIANT   0: chunk kernel only, 1: the round-1 micro-benchmark rule, 2: falls through to the chunk kernel, 3: 16-channel-slice DMA families
  int conv_s2_dma = 1;       // PT_CONV_S2_DMA    0: stride-2 3x3 layers on the register-staged 4 x 32 x 64 tile
  int conv_half = -1;        // PT_CONV_HALF      0 / 1: force the 8-wave / 4-wave tile, -1: the rule
  int n_group = -1;          // PT_N_GROUP        column tiles per L2 group of the 1x1 chunk kernels, 0: off, -1: the rule
  // read at every call (tests flip them inside one process)
  int conv1_wide = 1;        // PT_CONV1_WIDE     0: conv_igemm_kernel<1, 1> (one 32-channel chunk per stage) for every 1x1 stride-1 layer
  int conv_pipe = 4;         // PT_CONV_PIPE      0: v3 everywhere, 1: barrier behind tap 8, 2: in front of it (SKEW), 3: + register epilogue on plain layers, 4: + persistent workgroups, 5: persistent whatever the tile count
  int conv_pipe_blocks = 1;  // PT_CONV_PIPE_BLOCKS  0: the register-staged kernels for the 4- and 8-row maps
  int conv_ws64 = 1;         // PT_CONV_WS64      0: never, 1: the tile-count rule, 2: any tile count
  int conv_ws64_grid = 0;    // PT_CONV_WS64_GRID     > 0: at most this many workgroups (tests: longer tile runs)
  int conv_persist_grid = 0; // PT_CONV_PERSIST_GRID  > 0: this many workgroups (tests: longer runs)
  int conv_block_list = 1;   // PT_CONV_BLOCK_LIST 0: one image's 64 columns per workgroup of the 4 x 64 patch
  int conv_xp = kUnset;      // PT_CONV_XP        0 / 1: whole-line stores off / on everywhere, unset: the layer's own xp_store
  int gemm_pipe = 1;         // PT_GEMM_PIPE      0: the 4 x 32 x 64 tile kernels for the K >= 512 GEMMs
  int gemm_xp = 1;           // PT_GEMM_XP        0: 16-byte runs straight from the accumulators
  int lore_hm_fuse = 1;      // PT_LORE_HM_FUSE   0: hm.0 and hm.2 as two launches

  // get(name) -> the switch's text or null: getenv for the library, the tool's own settings for tools/conv_pick.cpp
  template <class Get>
  void parse_once(Get get) {
    set(conv1_direct, get("PT_CONV1_DIRECT"));
    set(conv_dma, get("PT_CONV_DMA"));
    set(conv_variant, get("PT_CONV_VARIANT"));
    set(conv_s2_dma, get("PT_CONV_S2_DMA"));
    set(conv_half, get("PT_CONV_HALF"));
    set(n_group, get("PT_N_GROUP"));
  }
  template <class Get>
  void parse_per_call(Get get) {
    set(conv1_wide, get("PT_CONV1_WIDE"));
    set(conv_pipe, get("PT_CONV_PIPE"));
    set(conv_pipe_blocks, get("PT_CONV_PIPE_BLOCKS"));
    set(conv_ws64, get("PT_CONV_WS64"));
    set(conv_ws64_grid, get("PT_CONV_WS64_GRID"));
    set(conv_persist_grid, get("PT_CONV_PERSIST_GRID"));
    set(conv_block_list, get("PT_CONV_BLOCK_LIST"));
    set(conv_xp, get("PT_CONV_XP"));
    set(gemm_pipe, get("PT_GEMM_PIPE"));
    set(gemm_xp, get("PT_GEMM_XP"));
    set(lore_hm_fuse, get("PT_LORE_HM_FUSE"));
  }
  // the process's environment: the first group at the first call only, the second at every call
  static ConvSwitches read() {
    static const ConvSwitches once = [] {
      ConvSwitches s;
      s.parse_once(getenv);
      return s;
    }();
    ConvSwitches s = once;
    s.parse_per_call(getenv);
    return s;
  }

 private:
  static void set(int& field, const char* text) {
    if (text) field = atoi(text);
  }
};

// ---- the layer, as far as the choice depends on it --------------------------------------------------------------------------------------
struct ConvShape {
  int B = 0, H = 0, W = 0, Cin = 0, N = 0, ks = 3, stride = 1;
  int rep = 1, shuffle_cout = 0, res_mode = 0, relu = 0, pool = 0, split = 0, nseg = 1, n_valid = 0, xp_store = 0;
  int pick_B = 0, pick_Ho = 0;      // ConvDesc.pick_B / pick_Ho: the extent the tile counts are taken over (0 = the launch's own)
  unsigned tap_mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool has_res = false, has_res_f32 = false, has_out_f32 = false, has_ylimit = false, has_xlimit = false, has_xlimit_rows = false,
       has_block_list = false, has_head_w = false, has_argmax_part = false, has_hm_w2 = false;
  int Ho() const { return (H + 2 * (ks / 2) - ks) / stride + 1; }
  int Wo() const { return (W + 2 * (ks / 2) - ks) / stride + 1; }
};

// ---- the choice -------------------------------------------------------------------------------------------------------------------------
enum class ConvFamily {
  chunk,            // conv_igemm_kernel<KS, STRIDE, GEOM, NHALF, DIRECT, F16>: register-staged 32-channel chunks (v1), every layer nothing else takes
  wide1,            // conv1x1_wide_kernel<KG, STAGED, GEN>: 1x1 stride 1, KG chunks per stage
  dma16,            // conv3x3_dma16_kernel<NT, NWV, S>: 16-channel-slice DMA (v3)
  pipe,             // conv3x3_pipe_kernel<NT, NWV, SKEW, BR, DIRECT, S, PHASE>: v3's tile with a software-pipelined tap loop (v4)
  pipe_persist,     // conv3x3_pipe_persist_kernel<NT, NWV, S>: the persistent form of pipe<NT, NWV, true, 0, true, S> (v5)
  pipe_persist_hm,  // conv3x3_pipe_persist_hm_kernel<2, 8, 1>: v5 with Lore's 256 -> 2 heat-map layer in its epilogue
  gemm_pipe,        // gemm_pipe_kernel<LIST>: 1x1 stride 1 with K >= 512 as a pipelined GEMM
  ws64,             // conv3x3_ws64_kernel: weight-stationary persistent 64 -> 64
};

struct ConvPick {
  ConvFamily family = ConvFamily::chunk;
  // the instance's template arguments (those of the family; the others keep these defaults)
  int NT = 0, NWV = 0, BR = 0, S = 1;                        // dma16 / pipe / pipe_persist(_hm)
  bool SKEW = false, DIRECT = false, PHASE = false;         // pipe; DIRECT (register epilogue) also chunk
  int KS = 0, STRIDE = 0, GEOM = 0, NHALF = 2;              // chunk (wide1 labels itself with KS = STRIDE = 1)
  bool F16 = false;
  int KG = 0;                                               // wide1
  bool STAGED = false, GEN = false;
  // what the choice also fixes in the kernel's argument block
  bool use_blist = false;      // ConvK.blist = the layer's block_list (gemm_pipe: the LIST instance)
  int n_group = 0, xp_store = 0, reps = 0;
};

inline bool conv_masked(const ConvShape& d) {
  for (int i = 0; i < 8; ++i)
    if (d.tap_mask[i]) return true;
  return false;
}
// the phase convolutions (db_model.hip phase_masks: four 64-channel tiles, taps (dy .. dy + 1) x (dx .. dx + 1)) have their own v4 variant
inline bool conv_phase_masked(const ConvShape& d) {
  bool phase = conv_masked(d) && d.N == 256;
  for (int i = 0; i < 8 && phase; ++i) {
    unsigned mk = 0;
    if (i < 4)
      for (int r = i >> 1; r < (i >> 1) + 2; ++r)
        for (int q = i & 1; q < (i & 1) + 2; ++q) mk |= 1u << (r * 3 + q);
    phase = d.tap_mask[i] == mk;
  }
  return phase;
}

// output rows of a dma16 / pipe / pipe_persist tile (32 columns wide, 64 * NT channels): 32 (NT 1, 8 waves), 16 (NT 2, or 4 waves), 8 (stride 2)
constexpr int conv_dma_tile_rows(int NT, int NWV, int S) { return (NT == 1 ? NWV : NWV / 2) * (S == 1 ? 4 : 2); }
// THE tile count of the selection rules: th x 32 pixel tiles of B maps of Ho x Wo (th = 16: the ws64 tile and the 128-channel DMA tile, 32: the 64-channel one)
inline long long conv_pixel_tiles(int B, int Ho, int Wo, int th) { return (long long)B * ((Ho + th - 1) / th) * ((Wo + 31) / 32); }

// the tile-count rule of the weight-stationary 64 -> 64 kernel, apart from the layer's own properties
inline bool conv_takes_ws64(const ConvSwitches& sw, int num_cu, int B, int Ho, int Wo) {
  return sw.conv_ws64 && (sw.conv_ws64 == 2 || conv_pixel_tiles(B, Ho, Wo, 16) >= 4ll * num_cu);
}
// the fused heat-map head is a form of the persistent tile: single-pass storage and none of the switches that select an earlier family
inline bool conv_fuses_hm(const ConvSwitches& sw, bool split) {
  return !split && sw.conv_dma && sw.conv_variant == 3 && sw.conv_pipe >= 4 && sw.lore_hm_fuse != 0;
}

// the chunk kernel's instance for a layer no other family took (wide1 where it applies)
inline void conv_pick_chunk(const ConvShape& d, const ConvSwitches& sw, int GEOM, ConvPick& p) {
  p.family = ConvFamily::chunk;
  p.KS = d.ks; p.STRIDE = d.stride; p.GEOM = GEOM; p.NHALF = 2;
  if (d.has_ylimit) {      // mostly empty worst-case extents: 16 tiles per workgroup
    p.reps = 16;
    p.n_group = 0;
  }
  const bool s1 = d.stride == 1 && GEOM == 0;
  // PT_CONV1_DIRECT=0: the staged epilogue for every launch of this kernel (A/B switch)
  const bool plain = sw.conv1_direct && GEOM == 0 && !d.split && !d.pool && !d.has_head_w && !d.has_argmax_part && !d.has_res_f32 && !d.shuffle_cout;
  const bool narrow = d.ks == 3 && s1 && d.n_valid > 0 && d.n_valid <= 32 && d.N == 64 && !d.split && !d.pool && !d.has_head_w &&
                      !d.has_argmax_part;      // <= 32 real output channels: half-width variant
  // every 1x1 stride-1 layer but the split / pooled ones: row-limited, Cin % 64 != 0 and the staged epilogues included
  // (Cin = 32 stays on the chunk kernel: one chunk is one stage either way, and the padded 2-chunk stage measured slower, 0.31 -> 0.37 ms @256x256)
  const bool wide1 = d.ks == 1 && s1 && !d.split && !d.pool && d.Cin >= 64 && sw.conv1_wide;
  if (narrow) {
    p.NHALF = 1;
    p.DIRECT = plain;
  } else if (wide1) {
    p.family = ConvFamily::wide1;
    p.STAGED = !plain;
    p.KG = d.Cin % 128 == 0 ? 4 : 2;      // KG = 4 where Cin is a multiple of 128, else 2 (zero-padded last stage where Cin is an odd number of 32-channel chunks)
    p.GEN = d.has_ylimit || d.Cin % 64 != 0;
  } else if (plain) {      // layers with a plain epilogue: the register-epilogue instances (1x1, stride-2 3x3, 3x3)
    p.DIRECT = true;
  } else {
    p.F16 = d.split == 2;
  }
}

inline ConvPick conv_pick(const ConvShape& d, int num_cu, const ConvSwitches& sw) {
  ConvPick p;
  const int Ho = d.Ho(), Wo = d.Wo();
  // the extent the tile counts below are taken over (ConvDesc.pick_B / pick_Ho)
  const int pB = d.pick_B > 0 ? d.pick_B : d.B, pHo = d.pick_Ho > 0 ? d.pick_Ho : Ho;
  const bool masked = conv_masked(d);
  const bool dma = sw.conv_dma != 0;
  const int pv = sw.conv_pipe;
  // PT_CONV_BLOCK_LIST=0: one image's 64 columns per workgroup (A/B switch, read per call)
  p.use_blist = d.has_xlimit && d.has_block_list && d.ks == 3 && d.stride == 1 && Ho <= 4 && Wo > 32 && Wo % 32 == 0 && sw.conv_block_list != 0;
  // the layer asks for it (ConvDesc.xp_store: the detector's graph, +0.9 % det-only; the layout net's many small hardswish GEMMs lose
  // 1.9 % to the extra barrier, the table nets are indifferent); PT_CONV_XP=0 / 1 forces it off / on everywhere (A/B switch, read per call)
  p.xp_store = (sw.conv_xp != ConvSwitches::kUnset ? sw.conv_xp : d.xp_store) && !d.has_out_f32;

  if (d.has_hm_w2) {      // hm.0 + hm.2 in one launch: the caller asked conv_fuses_hm; pt_launch_conv refuses anything but the plain 64 -> 256 + ReLU layer
    p.family = ConvFamily::pipe_persist_hm;
    p.NT = 2; p.NWV = 8; p.S = 1;
    return p;
  }
  // stride-2 3x3 layers with 128-wide output blocks (ResNet-18 / DLA-34 down-sampling convs): the 16-channel-slice DMA kernel on an 8 x 32 x 128 tile
  // (PT_CONV_S2_DMA=0: the register-staged 4 x 32 x 64 tile, A/B switch; PT_CONV_PIPE=0: the v3 stride-2 tile)
  if (d.ks == 3 && d.stride == 2 && !d.split && d.N % 128 == 0 && d.Cin % 32 == 0 && d.Cin >= 64 && pHo >= 8 && !d.has_head_w && !d.has_argmax_part && !d.n_valid &&
      !d.has_out_f32 && !d.has_res_f32 && !d.has_res && d.relu < 2 && !d.has_ylimit && !d.has_xlimit && !d.has_xlimit_rows && !d.pool && d.rep == 1 && !d.shuffle_cout &&
      dma && sw.conv_s2_dma && !masked) {
    p.NT = 2; p.NWV = 8; p.S = 2;
    if (pv != 0) { p.family = ConvFamily::pipe; p.SKEW = true; p.DIRECT = true; }
    else p.family = ConvFamily::dma16;
    return p;
  }
  if (d.ks == 3 && d.stride == 1 && !d.has_head_w && !d.has_argmax_part && !d.n_valid && !d.has_out_f32 && !d.has_res_f32 && d.relu < 2 && !d.has_ylimit && !d.has_xlimit &&
      !d.pool && d.split != 2 && dma) {
    // steady-state A/B on MI355X (tools/ab3.sh, round 1): the 16-channel-slice DMA kernel (v3) wins on >= 120-row maps
    // with K >= 128 channels, the 32-channel-slice DMA kernel (v2) on 60..119-row maps, the register-staged kernel
    // (v1) on short-K layers and on small maps, where the big DMA tiles leave CUs idle.
    // PT_CONV_VARIANT: 0 = v1 only, 1 = micro-benchmark rule, 2 = v2 wherever it applied (that kernel is gone: v1), 3 = v3 wherever it applies (default).
    // History: in the DB-ResNet18 graph at 8-page micro-batches v1-only measured fastest (det-only, no post: 3836 pages/s vs
    // 3764 with rule 1 and 3719 with v2) and was the default for most of round 1.  With 32-page det and 80-table Lore
    // micro-batches the 16-channel-slice DMA kernel wins where it applies (tools/ab_env.sh, two alternating runs each:
    // det-only 3503 / 3607 -> 3685 / 3647 pages/s, TSR-only 833 / 842 -> 845 / 859, four stages 354 / 358 -> 361 / 361).
    const int cv = sw.conv_variant;
    // plain 64 -> 64 layers with enough tiles to give every CU a run of them: the weight-stationary persistent kernel
    // (PT_CONV_WS64=0: the v3 tiles, A/B switch)
    if (cv == 3 && !d.split && d.Cin == 64 && d.N == 64 && d.rep == 1 && !d.shuffle_cout && d.res_mode <= 1 && !masked && conv_takes_ws64(sw, num_cu, pB, pHo, Wo)) {
      p.family = ConvFamily::ws64;
      return p;
    }
    const bool nt2 = d.N % 128 == 0;
    const bool v3ok = nt2 ? pHo >= 12 : pHo >= 24;
    const bool pick3 = (cv == 3 && v3ok) || (cv == 1 && d.Cin >= 128 && Ho >= 120);
    // the launch's tiles on the 8-wave tiling
    const long long tiles = conv_pixel_tiles(pB, pHo, Wo, nt2 ? 16 : 32) * (d.N / (nt2 ? 128 : 64));
    // 4-wave workgroups (16x32 pixels x 64 channels, 74 KB of LDS: two per CU) where the 8-wave tile is mostly prologue and
    // epilogue: short K (Cin <= 128: +3..8 % on 64->64 @240^2 / @256^2, 128->128 @120^2 / @128^2, 64->256 @256^2), and grids
    // that leave the 8-wave tiling with a ragged last round (512->512 @32^2 x 44: +12 %); K >= 2304 layers whose grid is whole
    // rounds stay on the 8-wave tiles (512->512 @30^2 x 32: -3 % as 4-wave).  PT_CONV_HALF = 0 / 1 forces one of them.
    const int half = sw.conv_half;
    bool use_half = half == 1;
    if (half < 0 && pick3) use_half = d.Cin <= 128 || (tiles < 2ll * num_cu && tiles % num_cu != 0);
    if (conv_phase_masked(d) && cv == 3 && v3ok && pv >= 3) {
      p.family = ConvFamily::pipe;
      p.NT = 2; p.NWV = 8; p.SKEW = true; p.PHASE = true;
      return p;
    }
    // v4 (software-pipelined tap loop) for the unmasked layers; PT_CONV_PIPE=0: v3 everywhere (A/B switch, read per call)
    const int pipe = masked ? 0 : pv;
    if (pick3) {
      // register epilogue for the plain layers (PT_CONV_PIPE=2: the staged fp32 epilogue everywhere, A/B switch)
      const bool direct = pipe >= 3 && !d.split && !d.pool && !d.shuffle_cout;
      // (a four-slice layer without a residual is better off on the persistent 8-wave tile than on the 4-wave one: 64 -> 256 @256^2 900 -> 955 TF/s; with
      // eight slices the two are level -- 128 -> 128 @128^2 1101 / 1120 -- and with a residual the 4-wave tile wins, 922 against 862)
      if (use_half && half < 0 && direct && pipe >= 4 && d.Cin == 64 && nt2 && !d.has_res && tiles >= 2ll * num_cu) use_half = false;
      p.NT = use_half ? 1 : (nt2 ? 2 : 1);
      p.NWV = use_half ? 4 : 8;
      // 4: the persistent form for the 8-wave tiles where a workgroup gets at least two tiles (interleaved A/B, tools/conv_ab.py: 256 -> 256 @64^2 1305 -> 1327
      // TF/s, @60^2 1174 -> 1198, 512 -> 512 @32^2 1379 -> 1404, @30^2 1267 -> 1275; the 4-wave tile LOSES 14 % as a persistent kernel -- 128 -> 128 @128^2
      // 1134 -> 975: two of its workgroups per CU already cover each other's prologues, and the run's bookkeeping costs it registers it does not have)
      // (5: whatever the tile count, and the 4-wave layers on the 8-wave persistent tile -- tests)
      if (direct && pipe >= 4 && (!use_half || pipe >= 5) && !d.has_xlimit && !d.has_xlimit_rows && !p.use_blist && (tiles >= 2ll * num_cu || pipe >= 5)) {
        p.family = ConvFamily::pipe_persist;
        p.NT = nt2 ? 2 : 1; p.NWV = 8;
      } else if (pipe >= 1) {
        p.family = ConvFamily::pipe;
        p.SKEW = pipe >= 2;
        p.DIRECT = direct;
      } else {
        p.family = ConvFamily::dma16;
      }
      return p;
    }
  }
  // maps that are exactly 4 or 8 rows high with K >= 1152 and 128-wide output blocks (the CRNN conv2.* / conv3.* layers): the pipelined DMA kernel on
  // tiles of four 4 x 32 / two 8 x 32 blocks -- from the compacted list of live blocks when the layer has one (PT_CONV_PIPE_BLOCKS=0: the
  // register-staged kernels, A/B switch read per call)
  if (d.ks == 3 && d.stride == 1 && (Ho == 4 || Ho == 8) && d.H == Ho && Wo % 32 == 0 && Wo > 32 && d.N % 128 == 0 && d.Cin >= 128 && !d.has_head_w &&
      !d.has_argmax_part && !d.n_valid && !d.has_out_f32 && !d.has_res_f32 && !d.has_res && d.relu < 2 && !d.has_ylimit && !d.has_xlimit_rows && d.rep == 1 &&
      !d.shuffle_cout && d.split != 2 && dma && !masked && sw.conv_pipe_blocks != 0 && pv != 0) {
    p.family = ConvFamily::pipe;
    p.NT = 2; p.NWV = 8; p.SKEW = true; p.BR = Ho;
    p.DIRECT = !d.split && !d.pool && pv >= 3;      // plain layer: register epilogue
    if (d.has_xlimit && d.has_block_list) p.use_blist = true;      // (8-row maps too: the 4 x 64 patch's rule above only takes lists for <= 4 rows)
    return p;
  }
  if (d.ks == 3) {      // the 4 x 64 patch for maps of at most 4 rows that are wider than one tile
    conv_pick_chunk(d, sw, d.stride == 1 && Ho <= 4 && Wo > 32 ? 1 : 0, p);
    return p;
  }
  // (K >= 512: at K = 256 a tile is four slices -- mostly prologue and epilogue of a workgroup that has the CU to itself -- and the 2048-wide
  // projection measured 1.65 ms against the streaming row GEMM's 1.42; K = 512 ... 1024: 1.43 -> 1.35, 0.70 -> 0.60, 0.42 -> 0.34, 1.17 -> 0.63 ms)
  // PT_GEMM_PIPE=0: the 4 x 32 x 64 tile kernels (A/B switch, read per call)
  if (d.ks == 1 && d.stride == 1 && !d.split && d.nseg <= 1 && d.Cin >= 512 && d.Cin % 64 == 0 && d.N % 128 == 0 && ((long long)d.B * d.H * d.W) % 32 == 0 &&
      !d.has_head_w && (!d.has_argmax_part || (!d.has_res && !d.relu)) && !d.has_res_f32 && !d.shuffle_cout && !d.pool && !d.has_ylimit && !d.has_xlimit && d.rep == 1 &&
      (!d.has_res || d.res_mode == 1) && (!d.has_xlimit_rows || (d.has_block_list && d.W % 32 == 0)) && dma && sw.gemm_pipe != 0) {
    p.family = ConvFamily::gemm_pipe;
    p.use_blist = d.has_xlimit_rows;
    p.xp_store = sw.gemm_xp != 0 && !d.has_out_f32;      // PT_GEMM_XP=0: 16-byte runs straight from the accumulators (A/B switch, read per call)
    return p;
  }
  {
    // column tiles per group: ~2 MB of weights (half of an XCD's L2); PT_N_GROUP overrides (0 = off)
    const long long tile_bytes = 64ll * d.Cin * 2 * (d.split == 2 ? 2 : (d.split ? 3 : 1));
    int g = sw.n_group >= 0 ? sw.n_group : (int)((2ll << 20) / tile_bytes);
    if (g < 1) g = sw.n_group == 0 ? 0 : 1;
    p.n_group = g;
  }
  conv_pick_chunk(d, sw, 0, p);
  return p;
}

// ---- the grid of a pick -----------------------------------------------------------------------------------------------------------------
struct ConvGrid {
  int tiles_x = 0, tiles_y = 0, n_tiles = 0;      // ConvK.tiles_x / tiles_y / n_tiles
  int total_tiles = 0;                            // ConvK.total_tiles (the families whose workgroups walk several tiles; else 0)
  long long count = 0, limit = 1ll << 31;         // what must lie in (0, limit): the blocks or tiles of the worst case
  long long nblk = 0;                             // workgroups launched
};

inline ConvGrid conv_pick_grid(const ConvShape& d, const ConvPick& p, int num_cu, const ConvSwitches& sw) {
  ConvGrid g;
  const int Ho = d.Ho(), Wo = d.Wo();
  int th = 0, tw = 32, nw = 64;
  switch (p.family) {
    case ConvFamily::chunk:
    case ConvFamily::wide1:
      tw = p.GEOM ? 64 : 32;
      th = p.GEOM ? 4 : ((d.stride == 1 && d.ks == 3) ? 8 : 4);
      break;
    case ConvFamily::ws64: th = 16; nw = d.N; break;
    case ConvFamily::gemm_pipe: nw = 128; break;
    default: th = conv_dma_tile_rows(p.NT, p.NWV, p.S); nw = 64 * p.NT; break;
  }
  g.n_tiles = d.N / nw;
  const int nblocks = p.family == ConvFamily::pipe && p.BR ? th / p.BR : (p.family == ConvFamily::chunk && p.GEOM == 1 && p.use_blist ? 2 : 1);
  if (p.family == ConvFamily::gemm_pipe) {      // 16 groups of 32 rows per workgroup; worst case with a list: every group live
    g.tiles_x = (int)(((long long)d.B * d.H * d.W / 32 + 15) / 16);
    g.tiles_y = 1;
    g.count = (long long)g.tiles_x * g.n_tiles;
  } else if (nblocks > 1 && p.use_blist) {      // live 32-column blocks, nblocks per workgroup: the worst case is every block of every image
    g.tiles_x = (int)(((long long)d.B * (Wo / 32) + nblocks - 1) / nblocks);
    g.tiles_y = 1;
    g.count = (long long)g.tiles_x * g.n_tiles;
  } else if (nblocks > 1) {                     // nblocks consecutive column blocks of one image
    g.tiles_x = (Wo + nblocks * 32 - 1) / (nblocks * 32);
    g.tiles_y = 1;
    g.count = (long long)d.B * g.tiles_x * g.n_tiles;
  } else {
    g.tiles_x = (Wo + tw - 1) / tw;
    g.tiles_y = (Ho + th - 1) / th;
    g.count = (long long)d.B * g.tiles_x * g.tiles_y * g.n_tiles;
  }
  g.nblk = g.count;
  switch (p.family) {
    case ConvFamily::chunk:
    case ConvFamily::wide1:
      if (p.reps > 1) {
        g.total_tiles = (int)g.count;
        g.nblk = (g.count + p.reps - 1) / p.reps;
      }
      break;
    case ConvFamily::pipe_persist:
    case ConvFamily::pipe_persist_hm: {      // one workgroup's LDS per CU; a heat-map workgroup's run is whole pixel tiles
      const long long most = p.family == ConvFamily::pipe_persist_hm ? g.count / (g.n_tiles ? g.n_tiles : 1) : g.count;
      g.total_tiles = (int)g.count;
      g.nblk = sw.conv_persist_grid > 0 ? sw.conv_persist_grid : num_cu;      // PT_CONV_PERSIST_GRID (tests): fewer workgroups, longer runs
      if (g.nblk > most) g.nblk = most;
      break;
    }
    case ConvFamily::ws64:      // one workgroup per CU walks total_tiles / grid tiles
      g.limit = 1ll << 30;
      g.total_tiles = (int)g.count;
      g.nblk = g.count < num_cu ? g.count : num_cu;
      if (sw.conv_ws64_grid > 0 && sw.conv_ws64_grid < g.nblk) g.nblk = sw.conv_ws64_grid;      // PT_CONV_WS64_GRID (tests): fewer workgroups, longer tile runs
      break;
    default: break;
  }
  return g;
}

// ---- names ------------------------------------------------------------------------------------------------------------------------------
constexpr int kConvLabelLen = 48;      // PtProfile's label width: longer labels are cut here, as they always were

// the profile label of a pick: bench.py's by_class and the tests parse these.  Returns the length the whole label has (snprintf's).
inline int conv_pick_label(const ConvShape& d, const ConvPick& p, char (&label)[kConvLabelLen]) {
  const int Ho = d.Ho(), Wo = d.Wo();
  const char* s2 = p.S == 2 ? "s2 " : "";
  const char* h = p.NWV == 4 ? "h" : "";
  const char* x3 = d.split ? " x3" : "";
  int n = 0;
  switch (p.family) {
    case ConvFamily::chunk:
    case ConvFamily::wide1:
      n = snprintf(label, sizeof(label), "conv%dx%d s%d %d->%d @%dx%d%s", d.ks, d.ks, d.stride, d.Cin, d.N, Ho, Wo, d.has_head_w ? " +head" : (d.split == 2 ? " h2" : x3));
      break;
    case ConvFamily::dma16:
      n = snprintf(label, sizeof(label), "conv3x3 %sv3%s %d->%d @%dx%d%s", s2, h, d.Cin, d.N, Ho, Wo, x3);
      break;
    case ConvFamily::pipe:
      if (p.BR) n = snprintf(label, sizeof(label), "conv3x3 v4b %d->%d @%dx%d%s", d.Cin, d.N, Ho, Wo, x3);
      else n = snprintf(label, sizeof(label), "conv3x3 %sv4%s%s %d->%d @%dx%d%s", s2, h, p.PHASE ? "p" : "", d.Cin, d.N, Ho, Wo, x3);
      break;
    case ConvFamily::pipe_persist:
      n = snprintf(label, sizeof(label), "conv3x3 %sv5%s %d->%d @%dx%d", s2, h, d.Cin, d.N, Ho, Wo);
      break;
    case ConvFamily::pipe_persist_hm:
      n = snprintf(label, sizeof(label), "conv3x3 v5+hm %d->%d->2 @%dx%d", d.Cin, d.N, Ho, Wo);
      break;
    case ConvFamily::gemm_pipe:
      if (d.has_argmax_part) n = snprintf(label, sizeof(label), "classifier gemm+argmax");      // (the label bench.py's by_class files the CTC classifier under)
      else n = snprintf(label, sizeof(label), "gemm %d->%d @%dx%d", d.Cin, d.N, Ho, Wo);
      break;
    case ConvFamily::ws64:
      n = snprintf(label, sizeof(label), "conv3x3 ws %d->%d @%dx%d", d.Cin, d.N, Ho, Wo);
      break;
  }
  return n;
}

// the instance as a kernel trace prints it: labels do not separate SKEW, DIRECT, BR = 4 / 8 or the chunk kernel's instances, this does
inline void conv_pick_kernel_name(const ConvPick& p, char* name, size_t n) {
  auto tf = [](bool b) { return b ? "true" : "false"; };
  switch (p.family) {
    case ConvFamily::chunk: snprintf(name, n, "conv_igemm_kernel<%d, %d, %d, %d, %s, %s>", p.KS, p.STRIDE, p.GEOM, p.NHALF, tf(p.DIRECT), tf(p.F16)); break;
    case ConvFamily::wide1: snprintf(name, n, "conv1x1_wide_kernel<%d, %s, %s>", p.KG, tf(p.STAGED), tf(p.GEN)); break;
    case ConvFamily::dma16: snprintf(name, n, "conv3x3_dma16_kernel<%d, %d, %d>", p.NT, p.NWV, p.S); break;
    case ConvFamily::pipe:
      snprintf(name, n, "conv3x3_pipe_kernel<%d, %d, %s, %d, %s, %d, %s>", p.NT, p.NWV, tf(p.SKEW), p.BR, tf(p.DIRECT), p.S, tf(p.PHASE));
      break;
    case ConvFamily::pipe_persist: snprintf(name, n, "conv3x3_pipe_persist_kernel<%d, %d, %d>", p.NT, p.NWV, p.S); break;
    case ConvFamily::pipe_persist_hm: snprintf(name, n, "conv3x3_pipe_persist_hm_kernel<%d, %d, %d>", p.NT, p.NWV, p.S); break;
    case ConvFamily::gemm_pipe: snprintf(name, n, "gemm_pipe_kernel<%s>", tf(p.use_blist)); break;
    case ConvFamily::ws64: snprintf(name, n, "conv3x3_ws64_kernel"); break;
  }
}
