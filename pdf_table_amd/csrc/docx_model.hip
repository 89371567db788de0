// docx_model.hip -- launch graph of DocXLayout's layout detector (DLASeg('dla34', down_ratio 4, head_conv 256) with eight heads).
//
// Reference graph: DLASeg.forward docx_layout/model_dla.py:617-652 (DocXLayoutModel, modeling_docxlayout.py)
//   base    = dla34 (the DLA of Lore's and CenterNet's detectors, dla_net.h)
//   dla_up  = DLAUp.forward :523-530 over IDAUp.forward :490-504 -- CenterNet's up-path, launch for launch (dla_up.h)
//   heads   = conv3x3(64->256) + bias + ReLU, conv1x1 -> k + bias for cls (4), ftype (3), hm (11), hm_sub (2), reg (2), reg_sub (2), wh (8), wh_sub (8)
//             (configuration_docxlayout.py:45-46)
// The heads are layered as CenterNet's are: ONE 256-channel hidden map, written by a head's 3x3 launch and read by its 1x1 launch, then reused by the
// next head (the launches of a stream are ordered).  Fusing the eight heads into one launch is not done here: at the model's 192 x 192 maps the hidden
// map's round trip (2 x 192^2 x 256 x 2 bytes = 38 MB per head and page) is small beside the heads' 87 GFLOP per page.
// The arena is the layout stage's (PT_ARENA_LAYOUT): a pipeline has its layout stage and its table stage (PT_ARENA_TSR) in flight together.
#include "dla_up.h"

namespace PT_FMT_NS {

// x: NHWC4 bf16 [n, H, W, 4] ([hi bgr0 | lo bgr0] in the pair modes); heads: fp32 NHWC at H/4 x W/4, pre-sigmoid; hm has channel stride 16
// (11 valid), every other head stride 8 (cls 4, ftype 3, hm_sub 2, reg 2, reg_sub 2, wh 8, wh_sub 8 valid)
int pt_docx_net(pt_engine* e, const bf16_t* x, int n, int H, int W, float* cls, float* ftype, float* hm, float* hm_sub, float* reg, float* reg_sub,
                float* wh, float* wh_sub, hipStream_t s) {
  PT_REQUIRE(H % 32 == 0 && W % 32 == 0 && H > 0 && W > 0, "DocXLayout net: input %dx%d must be multiples of 32", H, W);
  PT_REQUIRE(x && n > 0 && cls && ftype && hm && hm_sub && reg && reg_sub && wh && wh_sub, "DocXLayout net: null pointer");
  const PtModel* m = pt_find_model(e, PT_MODEL_DOCX_DLA34, "DocXLayout DLA-34", "PT_MODEL_DOCX_DLA34");
  if (!m) return PT_ERR_STATE;
  CCtx c;
  c.init(e, m, "DocXLayout DLA-34", s, n, PT_ARENA_LAYOUT);
  float* heads[8] = {cls, ftype, hm, hm_sub, reg, reg_sub, wh, wh_sub};
  const char* hname[8] = {"cls", "ftype", "hm", "hm_sub", "reg", "reg_sub", "wh", "wh_sub"};
  const int hreal[8] = {4, 3, 11, 2, 2, 2, 8, 8};
  return pt_plan_then_launch(c, "DocXLayout net", [&] {
    std::vector<T> layers = dla34_base(c, x, H, W);
    c.ida("dla_up.ida_0", layers, 4, 6, 256, true);
    c.ida("dla_up.ida_1", layers, 3, 6, 128, true);
    c.ida("dla_up.ida_2", layers, 2, 6, 64, false);
    const T feat = layers[5];
    T hid = c.alloc(feat.H, feat.W, 256);
    for (int h = 0; h < 8; ++h) {
      const int cs = hreal[h] > 8 ? 16 : 8;
      c.conv(feat, std::string(hname[h]) + ".0", 256, 3, 1, hid, 1);
      c.conv(hid, std::string(hname[h]) + ".2", 64, 1, 1, T(), 0, nullptr, cs, heads[h], cs, 0, hreal[h]);
    }
    return c.rc;
  });
}

}  // namespace PT_FMT_NS
