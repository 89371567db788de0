// conv_pick -- which kernel a dense convolution layer takes, without a GPU (pdf_table_amd/csrc/conv_pick.h is the whole rule).
//
//   c++ -std=c++17 -O1 -o tools/conv_pick tools/conv_pick.cpp
//   conv_pick [--num-cu 256] [NAME=VALUE ...] B H W Cin N ks stride      one layer from the command line; NAME: a switch (PT_CONV_PIPE=0)
//                                                                        or a further field of ConvShape (has_res=1 relu=1 split=1)
//   conv_pick [--num-cu 256] [NAME=VALUE ...] < rows.json                one JSON object per line (tests/golden/conv_pick/grid.json)
//   conv_pick --switches [PT_NAME=VALUE ...]                             the parsed switches, one "NAME value" per line
//
// A JSON row holds the fields of ConvShape by name (has_* as true / false or 0 / 1, tap_mask as an array), "num_cu", and the switches as
// "PT_NAME": "value" pairs; objects may be nested ({"shape": {...}, "switches": {...}}), the keys are taken flat.  Switches that neither the
// command line nor the row sets come from the environment.  Output per layer, tab-separated: label, kernel name, workgroups, tiles_x, tiles_y, n_tiles.
#include <ctype.h>
#include <string.h>

#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../pdf_table_amd/csrc/conv_pick.h"

typedef std::map<std::string, std::string> Settings;

// the flat "key": value pairs of one JSON line; a value is a number, a quoted string, true / false / null or an array of numbers (kept as "a,b,c")
static bool parse_row(const std::string& ln, Settings& kv) {
  size_t i = 0;
  const size_t n = ln.size();
  auto skip = [&] { while (i < n && (isspace((unsigned char)ln[i]) || ln[i] == ',' || ln[i] == '{' || ln[i] == '}')) ++i; };
  auto quoted = [&](std::string& out) {
    out.clear();
    for (++i; i < n && ln[i] != '"'; ++i) out += ln[i];
    if (i >= n) return false;
    ++i;
    return true;
  };
  for (skip(); i < n; skip()) {
    std::string key, val;
    if (ln[i] != '"' || !quoted(key)) return false;
    while (i < n && isspace((unsigned char)ln[i])) ++i;
    if (i >= n || ln[i] != ':') return false;
    for (++i; i < n && isspace((unsigned char)ln[i]); ++i) {}
    if (i >= n) return false;
    if (ln[i] == '{') continue;      // a nested object: its pairs follow
    if (ln[i] == '"') {
      if (!quoted(val)) return false;
    } else if (ln[i] == '[') {
      for (++i; i < n && ln[i] != ']'; ++i)
        if (!isspace((unsigned char)ln[i])) val += ln[i];
      if (i >= n) return false;
      ++i;
    } else {
      for (; i < n && ln[i] != ',' && ln[i] != '}' && !isspace((unsigned char)ln[i]); ++i) val += ln[i];
    }
    kv[key] = val;
  }
  return true;
}

static int as_int(const std::string& v) { return v == "true" ? 1 : (v == "false" || v == "null" ? 0 : atoi(v.c_str())); }

static bool shape_of(const Settings& kv, ConvShape& d, std::string& err) {
  const struct { const char* name; int* field; } ints[] = {
      {"B", &d.B}, {"H", &d.H}, {"W", &d.W}, {"Cin", &d.Cin}, {"N", &d.N}, {"ks", &d.ks}, {"stride", &d.stride}, {"rep", &d.rep},
      {"shuffle_cout", &d.shuffle_cout}, {"res_mode", &d.res_mode}, {"relu", &d.relu}, {"pool", &d.pool}, {"split", &d.split}, {"nseg", &d.nseg},
      {"n_valid", &d.n_valid}, {"xp_store", &d.xp_store}, {"pick_B", &d.pick_B}, {"pick_Ho", &d.pick_Ho}};
  const struct { const char* name; bool* field; } flags[] = {
      {"has_res", &d.has_res}, {"has_res_f32", &d.has_res_f32}, {"has_out_f32", &d.has_out_f32}, {"has_ylimit", &d.has_ylimit}, {"has_xlimit", &d.has_xlimit},
      {"has_xlimit_rows", &d.has_xlimit_rows}, {"has_block_list", &d.has_block_list}, {"has_head_w", &d.has_head_w}, {"has_argmax_part", &d.has_argmax_part},
      {"has_hm_w2", &d.has_hm_w2}};
  for (const auto& f : ints)
    if (auto it = kv.find(f.name); it != kv.end()) *f.field = as_int(it->second);
  for (const auto& f : flags)
    if (auto it = kv.find(f.name); it != kv.end()) *f.field = as_int(it->second) != 0;
  if (auto it = kv.find("tap_mask"); it != kv.end()) {
    const char* s = it->second.c_str();
    for (int i = 0; i < 8 && *s; ++i) {
      d.tap_mask[i] = (unsigned)strtoul(s, nullptr, 0);
      s += strcspn(s, ",");
      if (*s) ++s;
    }
  }
  // what pt_launch_conv requires before it picks
  if (d.B <= 0 || d.H <= 0 || d.W <= 0) err = "B, H, W must be positive";
  else if (d.Cin <= 0 || d.Cin % 32) err = "Cin must be a positive multiple of 32";
  else if (d.N <= 0 || d.N % 64) err = "N must be a positive multiple of 64";
  else if ((d.ks != 1 && d.ks != 3) || (d.stride != 1 && d.stride != 2)) err = "ks must be 1 or 3, stride 1 or 2";
  return err.empty();
}

static bool report(const Settings& kv, int num_cu) {
  ConvShape d;
  std::string err;
  if (!shape_of(kv, d, err)) {
    std::cerr << "conv_pick: " << err << "\n";
    return false;
  }
  if (auto it = kv.find("num_cu"); it != kv.end()) num_cu = as_int(it->second);
  auto get = [&](const char* name) -> const char* {
    auto it = kv.find(name);
    return it != kv.end() ? it->second.c_str() : getenv(name);
  };
  ConvSwitches sw;
  sw.parse_once(get);
  sw.parse_per_call(get);
  const ConvPick p = conv_pick(d, num_cu, sw);
  const ConvGrid g = conv_pick_grid(d, p, num_cu, sw);
  char label[kConvLabelLen], name[96];
  conv_pick_label(d, p, label);
  conv_pick_kernel_name(p, name, sizeof(name));
  std::cout << label << "\t" << name << "\t" << g.nblk << "\t" << g.tiles_x << "\t" << g.tiles_y << "\t" << g.n_tiles << "\n";
  return true;
}

int main(int argc, char** argv) {
  Settings base;
  std::vector<std::string> pos;
  int num_cu = 256;
  bool switches_only = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t eq = a.find('=');
    if (a == "--num-cu" && i + 1 < argc) num_cu = atoi(argv[++i]);
    else if (a == "--switches") switches_only = true;
    else if (eq != std::string::npos) base[a.substr(0, eq)] = a.substr(eq + 1);      // a switch (PT_CONV_PIPE=0) or a further field of the shape (has_res=1)
    else pos.push_back(a);
  }
  if (switches_only) {
    auto get = [&](const char* name) -> const char* {
      auto it = base.find(name);
      return it != base.end() ? it->second.c_str() : getenv(name);
    };
    ConvSwitches sw;
    sw.parse_once(get);
    sw.parse_per_call(get);
    const struct { const char* name; int v; } all[] = {
        {"PT_CONV1_DIRECT", sw.conv1_direct}, {"PT_CONV_DMA", sw.conv_dma}, {"PT_CONV_VARIANT", sw.conv_variant}, {"PT_CONV_S2_DMA", sw.conv_s2_dma},
        {"PT_CONV_HALF", sw.conv_half}, {"PT_N_GROUP", sw.n_group}, {"PT_CONV1_WIDE", sw.conv1_wide}, {"PT_CONV_PIPE", sw.conv_pipe},
        {"PT_CONV_PIPE_BLOCKS", sw.conv_pipe_blocks}, {"PT_CONV_WS64", sw.conv_ws64}, {"PT_CONV_WS64_GRID", sw.conv_ws64_grid},
        {"PT_CONV_PERSIST_GRID", sw.conv_persist_grid}, {"PT_CONV_BLOCK_LIST", sw.conv_block_list}, {"PT_CONV_XP", sw.conv_xp}, {"PT_GEMM_PIPE", sw.gemm_pipe},
        {"PT_GEMM_XP", sw.gemm_xp}, {"PT_LORE_HM_FUSE", sw.lore_hm_fuse}};
    for (const auto& s : all) {
      if (s.v == ConvSwitches::kUnset) std::cout << s.name << " unset\n";
      else std::cout << s.name << " " << s.v << "\n";
    }
    return 0;
  }
  if (!pos.empty()) {
    const char* names[7] = {"B", "H", "W", "Cin", "N", "ks", "stride"};
    if (pos.size() != 7) {
      std::cerr << "usage: conv_pick [--num-cu N] [NAME=VALUE ...] B H W Cin N ks stride   (or JSON rows on stdin; --switches)\n";
      return 2;
    }
    for (int i = 0; i < 7; ++i) base[names[i]] = pos[i];
    return report(base, num_cu) ? 0 : 1;
  }
  std::string ln;
  int rc = 0;
  while (std::getline(std::cin, ln)) {
    if (ln.find_first_not_of(" \t\r") == std::string::npos) continue;
    Settings kv = base;
    if (!parse_row(ln, kv)) {
      std::cerr << "conv_pick: cannot parse: " << ln << "\n";
      std::cout << "?\t?\t0\t0\t0\t0\n";      // (one output line per input line)
      rc = 1;
    } else if (!report(kv, num_cu)) {
      std::cout << "?\t?\t0\t0\t0\t0\n";
      rc = 1;
    }
  }
  return rc;
}
