// Test driver for the PCM method of include/afs_synthesizer.hpp (TdsVoices::synthesizeSignalTdsPcm).
// MockTube as in adapter_main.cpp: the members the adapter reads, no reference code.
//   adapter_pcm_main synth <in> <out>    run one voice over the frames of <in>, one PCM call per frame;
//                                        <out>: the int16 samples, then (after them) nothing else
//   adapter_pcm_main latency <in> <out>  two voices of the same seed on one context, called in turn per
//                                        frame -- the fp64 call, then the PCM call; <out>: doubles, per
//                                        frame the wall time (ms) of the fp64 call and of the PCM call
// <in>: int32 F, int32 hop, double fs, uint32 seed, then F afs_frame records (as adapter_main).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "afs_synthesizer.hpp"

struct MockTube {
  enum Articulator { VOCAL_FOLDS, TONGUE, LOWER_INCISORS, LOWER_LIP, OTHER_ARTICULATOR, NUM_ARTICULATORS };
  struct Section {
    double pos_cm, area_cm2, length_cm, volume_cm3, wallMass_cgs, wallStiffness_cgs, wallResistance_cgs;
    Articulator articulator;
    double laterality;
  };
  Section pharynxMouthSection[40];
  Section noseSection[19];
  double teethPosition_cm;
  double aspirationStrength_dB;
  double getVelumOpening_cm2() const { return noseSection[0].area_cm2; }
};

static void fill(MockTube &t, const afs_frame &f) {
  std::memset(&t, 0, sizeof t);
  for (int i = 0; i < 40; ++i) {
    t.pharynxMouthSection[i].area_cm2 = f.area_cm2[i];
    t.pharynxMouthSection[i].length_cm = f.length_cm[i];
    t.pharynxMouthSection[i].laterality = f.laterality[i];
    t.pharynxMouthSection[i].articulator = (MockTube::Articulator)f.articulator[i];
  }
  t.teethPosition_cm = f.teeth_position_cm;
  t.noseSection[0].area_cm2 = f.velum_opening_cm2;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const bool latency = !std::strcmp(argv[1], "latency");
  if (!latency && std::strcmp(argv[1], "synth")) return 2;
  FILE *fi = std::fopen(argv[2], "rb");
  if (!fi) return 3;
  int32_t F = 0, hop = 0;
  double fs = 0;
  uint32_t seed = 1;
  if (std::fread(&F, 4, 1, fi) != 1 || std::fread(&hop, 4, 1, fi) != 1 || std::fread(&fs, 8, 1, fi) != 1 ||
      std::fread(&seed, 4, 1, fi) != 1)
    return 3;
  std::vector<afs_frame> fr((size_t)F);
  if (std::fread(fr.data(), sizeof(afs_frame), (size_t)F, fi) != (size_t)F) return 3;
  std::fclose(fi);
  afs::Context ctx(fs);
  afs::TdsVoices<MockTube> voice(ctx, 1, &seed), voice64(ctx, 1, &seed);
  std::vector<short> pcm, buf((size_t)(hop < 1 ? 1 : hop));
  std::vector<double> ms, buf64(buf.size());
  using clk = std::chrono::steady_clock;
  auto msec = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  for (int k = 0; k < F; ++k) {
    MockTube t;
    fill(t, fr[(size_t)k]);
    if (latency) {
      const auto a0 = clk::now();
      voice64.synthesizeSignalTds(&t, fr[(size_t)k].glottis, hop, buf64.data());
      const auto a1 = clk::now();
      ms.push_back(msec(a0, a1));
    }
    const auto t0 = clk::now();
    const int n = voice.synthesizeSignalTdsPcm(&t, fr[(size_t)k].glottis, hop, buf.data());
    const auto t1 = clk::now();
    if (latency) ms.push_back(msec(t0, t1));
    pcm.insert(pcm.end(), buf.begin(), buf.begin() + n);
  }
  FILE *fo = std::fopen(argv[3], "wb");
  if (!fo) return 3;
  if (latency) std::fwrite(ms.data(), sizeof(double), ms.size(), fo);
  else std::fwrite(pcm.data(), sizeof(short), pcm.size(), fo);
  std::fclose(fo);
  std::printf("samples %zu\n", pcm.size());
  return 0;
}
