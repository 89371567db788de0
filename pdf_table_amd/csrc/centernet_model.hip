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
#include "dla_up.h"

namespace PT_FMT_NS {

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
