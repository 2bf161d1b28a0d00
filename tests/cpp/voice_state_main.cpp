// voice_state_main.cpp -- afs_voice_state.h on the CPU (tests/test_snapshot_cpu.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer): the record layout of a voice, the map from a
// record's 16-byte vectors to a session's buffers that the gather and scatter kernels use, and the header
// check.  Stand-in sessions of the real sizes (Lane<16>, Lane<64>, X_TOTAL, afs_frame) are filled with a
// pattern; two voices are packed into records and unpacked into other slots of a session of another
// batch size, vector by vector as the kernels do.  Prints "voice-state-ok", or the first property that
// fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "afs_voice_state.h"
#include "tree_core.h"

namespace {

using Bytes = std::vector<uint8_t>;

int fail(const char *name, const char *what, long at) {
  std::printf("%s: %s (at %ld)\n", name, what, at);
  return 1;
}

// a session's three buffers for B voices, every byte a function of (salt, buffer, offset)
struct Session {
  Bytes buf[afs::VOICE_STATE_PARTS];
  Session(const afs::VoiceStateLayout &L, int B, unsigned salt) {
    for (int p = 0; p < afs::VOICE_STATE_PARTS; ++p) {
      buf[p].resize((size_t)(B * L.stride[p]));
      for (size_t k = 0; k < buf[p].size(); ++k) buf[p][k] = (uint8_t)(salt + 17u * (unsigned)p + 131u * k + (k >> 8) + (k >> 16));
    }
  }
};

// the gather and the scatter on the host: every payload vector of every record through voice_state_vec
void gather(const afs::VoiceStateLayout &L, const Session &s, const std::vector<int32_t> &voices, Bytes &records) {
  for (size_t i = 0; i < voices.size(); ++i)
    for (int64_t v = 0; v < afs::voice_state_payload_vecs(L); ++v) {
      const afs::VoiceStateVec at = afs::voice_state_vec(L, v, voices[i]);
      if (at.part < 0) continue;
      std::memcpy(&records[i * (size_t)L.record_bytes + (size_t)at.record_off], &s.buf[at.part][(size_t)at.session_off], 16);
    }
}
void scatter(const afs::VoiceStateLayout &L, Session &s, const std::vector<int32_t> &voices, const Bytes &records) {
  for (size_t i = 0; i < voices.size(); ++i)
    for (int64_t v = 0; v < afs::voice_state_payload_vecs(L); ++v) {
      const afs::VoiceStateVec at = afs::voice_state_vec(L, v, voices[i]);
      if (at.part < 0) continue;
      std::memcpy(&s.buf[at.part][(size_t)at.session_off], &records[i * (size_t)L.record_bytes + (size_t)at.record_off], 16);
    }
}

int check_layout(const char *name, int lanes, int64_t lane_bytes) {
  const int64_t frame = (int64_t)sizeof(afs_frame);
  const afs::VoiceStateLayout L = afs::voice_state_layout(lanes, lane_bytes, afs::tree::X_TOTAL, frame);
  // the parts: 16-byte aligned, in order, none overlapping, whole vectors, the record no larger than they need
  int64_t at = (int64_t)sizeof(afs::VoiceStateHeader);
  const int64_t want[3] = {lanes * lane_bytes, (int64_t)afs::tree::X_TOTAL * 8, frame};
  for (int p = 0; p < afs::VOICE_STATE_PARTS; ++p) {
    if (L.bytes[p] != want[p]) return fail(name, "part size", p);
    if (L.bytes[p] % 16) return fail(name, "part not whole vectors", p);
    if (L.offset[p] % 16 || L.offset[p] != at) return fail(name, "part offset", p);
    at += afs::voice_state_pad16(L.bytes[p]);
  }
  if (L.record_bytes != at || L.record_bytes % 16) return fail(name, "record size", (long)L.record_bytes);
  if (L.stride[0] != L.bytes[0] || L.stride[1] != L.bytes[1] || L.stride[2] != 2 * frame) return fail(name, "stride", 0);
  if (afs::voice_state_payload_vecs(L) * 16 + (int64_t)sizeof(afs::VoiceStateHeader) != L.record_bytes)
    return fail(name, "payload vectors", (long)afs::voice_state_payload_vecs(L));

  // pack voices 3 and 1 of a session of 5
  const std::vector<int32_t> from = {3, 1}, to = {0, 2};
  const Session src(L, 5, 1u);
  Bytes records(from.size() * (size_t)L.record_bytes, 0xEE);
  gather(L, src, from, records);
  for (size_t i = 0; i < from.size(); ++i) {
    const uint8_t *rec = &records[i * (size_t)L.record_bytes];
    for (size_t k = 0; k < sizeof(afs::VoiceStateHeader); ++k)
      if (rec[k] != 0xEE) return fail(name, "gather wrote into the header", (long)k);
    for (int p = 0; p < afs::VOICE_STATE_PARTS; ++p)
      for (int64_t k = 0; k < L.bytes[p]; ++k)
        if (rec[L.offset[p] + k] != src.buf[p][(size_t)(from[i] * L.stride[p] + k)]) return fail(name, "payload byte", (long)k);
  }
  // unpack into voices 0 and 2 of a session of 4: those voices' parts are the sources', all else stays
  Session dst(L, 4, 99u);
  const Session before = dst;
  scatter(L, dst, to, records);
  for (int p = 0; p < afs::VOICE_STATE_PARTS; ++p)
    for (size_t k = 0; k < dst.buf[p].size(); ++k) {
      const int64_t u = (int64_t)k / L.stride[p], in = (int64_t)k % L.stride[p];
      int64_t i = -1;
      for (size_t q = 0; q < to.size(); ++q)
        if (to[q] == u && in < L.bytes[p]) i = (int64_t)q;  // (in >= bytes: pair[u][1], never written)
      const uint8_t wantb = i < 0 ? before.buf[p][k] : src.buf[p][(size_t)(from[(size_t)i] * L.stride[p] + in)];
      if (dst.buf[p][k] != wantb) return fail(name, i < 0 ? "a byte outside the destinations changed" : "destination byte", (long)k);
    }
  // and a record of what was unpacked equals the one it came from
  Bytes again(records.size(), 0xEE);
  gather(L, dst, to, again);
  if (again != records) return fail(name, "save(load(save)) differs", 0);
  return 0;
}

int check_header() {
  const char *name = "header";
  afs_options o{};
  o.turbulence_losses = o.soft_walls = o.generate_noise_sources = o.radiation_from_skin = o.inner_length_corrections = 1;
  o.flow_separation_area_ratio = 1.0;
  const afs::VoiceStateHeader own = afs::voice_state_header(16, 1024, 1032, 44100.0, o, false, 0);
  afs::VoiceStateHeader h = afs::voice_state_header(16, 1024, 1032, 44100.0, o, true, 77);
  if (afs::voice_state_mismatch(h, own)) return fail(name, "own record refused", 0);
  if (h.latched != 1 || h.seed != 77 || h.reserved != 0) return fail(name, "fields", 0);
  {  // every byte defined, the struct's padding included
    afs::VoiceStateHeader g = afs::voice_state_header(16, 1024, 1032, 44100.0, o, true, 77);
    if (std::memcmp(&g, &h, sizeof h)) return fail(name, "bytes differ between two equal headers", 0);
  }
  int n = 0;
  auto refused = [&](afs::VoiceStateHeader bad) { ++n; return afs::voice_state_mismatch(bad, own) != nullptr; };
#define CORRUPT(stmt)                                   \
  {                                                     \
    afs::VoiceStateHeader bad = h;                      \
    stmt;                                               \
    if (!refused(bad)) return fail(name, #stmt, n);     \
  }
  CORRUPT(bad.magic ^= 1u)
  CORRUPT(bad.version += 1)
  CORRUPT(bad.lanes = 64)
  CORRUPT(bad.x_total += 1)
  CORRUPT(bad.lane_bytes = 552)
  CORRUPT(bad.sampling_rate_hz = 22050.0)
  CORRUPT(bad.sampling_rate_hz = std::numeric_limits<double>::quiet_NaN())
  CORRUPT(bad.options.turbulence_losses ^= 1)
  CORRUPT(bad.options.soft_walls ^= 1)
  CORRUPT(bad.options.generate_noise_sources ^= 1)
  CORRUPT(bad.options.radiation_from_skin ^= 1)
  CORRUPT(bad.options.piriform_fossa ^= 1)
  CORRUPT(bad.options.inner_length_corrections ^= 1)
  CORRUPT(bad.options.transvelar_coupling ^= 1)
  CORRUPT(bad.options.glottis_loss = 2)
  CORRUPT(bad.options.glottis_model = 1)
  CORRUPT(bad.options.flow_separation_area_ratio = 1.2)
  CORRUPT(bad.latched = 2)
#undef CORRUPT
  // the voice's own fields are no mismatch
  h.latched = 0, h.seed = 0;
  if (afs::voice_state_mismatch(h, own)) return fail(name, "an unlatched record refused", 0);
  return 0;
}

}  // namespace

int main() {
  static_assert(sizeof(afs::VoiceStateHeader) % 16 == 0, "header");
  int bad = check_layout("16 lanes", 16, (int64_t)sizeof(afs::tree::Lane<16>));
  if (!bad) bad = check_layout("64 lanes", 64, (int64_t)sizeof(afs::tree::Lane<64>));
  if (!bad) bad = check_header();
  if (!bad) std::printf("voice-state-ok\n");
  return bad;
}
