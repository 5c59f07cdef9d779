// Stand-alone driver of the convolution plan (accflow_amd/csrc/conv_plan.cpp) for tests/test_conv_plan.py: host code only, built
// with the host compiler and the sanitizers, no GPU and no HIP runtime.  Reads accflow_conv_desc records from a file and prints
// one line of integers per descriptor:
//   index valid | slots norm                      - what accflow_conv_stat_slots / accflow_conv_in_norm_supported compute
//   | q: the plan with want_stats = true           - ok family tc tp wc wp lay loop tapgemm norm w4 mode slots ch0 Z
//   | s: the plan of the same descriptor with stats set and stat_slots = q.slots (validated again)
//   | l: the plan of the launch (want_stats = stats != NULL)
//   | the launch's parts: Z and outputs of the head and of the tail (0 0 0 0 without a tail split)
#include <stdio.h>
#include <string.h>

#include <vector>

#include "conv_plan.h"

static void print_plan(int ok, const conv_plan& p) {
  if (!ok) { printf(" | 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0"); return; }
  printf(" | 1 %d %d %d %d %d %d %d %d %d %d %d %d %d %d", p.family, p.tc, p.tp, p.wc, p.wp, p.lay, p.loop, (int)p.tapgemm, (int)p.norm,
         (int)p.w4, p.mode, p.slots, p.ch0, p.Z);
}

static int plan_of(const accflow_conv_desc& desc, bool want_stats, conv_plan& p) {
  accflow_conv_desc d;
  return !conv_validate(&desc, d) && !conv_make_plan(d, want_stats, p);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: conv_plan_driver <descriptors.bin>\n"); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  std::vector<accflow_conv_desc> descs;
  accflow_conv_desc rec;
  while (fread(&rec, sizeof(rec), 1, f) == 1) descs.push_back(rec);
  fclose(f);
  static float dummy_stats;
  for (size_t i = 0; i < descs.size(); ++i) {
    const accflow_conv_desc& desc = descs[i];
    accflow_conv_desc d;
    const int valid = !conv_validate(&desc, d);
    conv_plan q = conv_plan(), s = conv_plan(), l = conv_plan(), n = conv_plan();
    const int qok = plan_of(desc, true, q);
    accflow_conv_desc probe = desc;
    probe.in_norm = nullptr;
    probe.stats = nullptr;
    const int nok = plan_of(probe, false, n);
    const bool plain = desc.epi == ACCFLOW_EPI_STORE && desc.act == ACCFLOW_ACT_NONE;
    printf("%zu %d | %d %d", i, valid, plain && qok ? q.slots : 0, nok && n.can_norm ? 1 : 0);
    print_plan(qok, q);
    accflow_conv_desc with = desc;
    with.stats = &dummy_stats;
    with.stat_slots = q.slots;
    const int sok = qok && plan_of(with, true, s);
    print_plan(sok, s);
    // the launch: its descriptor is the validated copy, completed by the planner
    int lok = valid && !conv_make_plan(d, d.stats != nullptr, l);
    print_plan(lok, l);
    long long part[4] = {0, 0, 0, 0};
    if (lok && l.ch0) {
      accflow_conv_desc h, t;
      conv_tail_split(d, l.ch0, h, t);
      conv_plan ph, pt;
      if (conv_plan_part(h, l, false, ph) || conv_plan_part(t, l, true, pt)) lok = -1;
      part[0] = ph.Z; part[1] = (long long)h.B * h.Cout * h.OH * h.OW;
      part[2] = pt.Z; part[3] = (long long)t.B * t.Cout * t.OH * t.OW;
      if (h.Cout + t.Cout != d.Cout || t.Cout <= 0 || t.Cout > 64 || (h.Cout % 128)) lok = -1;
    }
    printf(" | %d %lld %lld %lld %lld\n", lok, part[0], part[1], part[2], part[3]);
  }
  return 0;
}
