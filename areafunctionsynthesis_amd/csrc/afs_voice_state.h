// afs_voice_state.h -- the record of one voice's state outside its session slot (afs_session_save_voices,
// afs_session_load_voices, afs_session_copy_voices).  Host and device: the layout, the map
// from a record's 16-byte vectors to the session's buffers that the gather and scatter kernels use
// (session_kernels.hip), and the header that the host writes and checks (afs_capi.cpp).  Depends on
// include/afs.h alone, so a CPU program can compile it (tests/cpp/voice_state_main.cpp).
//
//   [ VoiceStateHeader | Lane<W>[W] | X_TOTAL doubles | afs_frame ]     each part padded to 16 bytes
//
// The payload is the voice's device bytes, verbatim: its lane registers (afs_session::tree_lanes), its
// saved LDS image (afs_session::ws) and its latched frame pair[u][0].
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/afs.h"

#if defined(__HIPCC__)
#define AFS_VS_HD __host__ __device__
#else
#define AFS_VS_HD
#endif

namespace afs {

constexpr uint32_t VOICE_STATE_MAGIC = 0x53564641u;  // "AFVS"
constexpr uint32_t VOICE_STATE_VERSION = 1;          // of this layout

struct VoiceStateHeader {
  uint32_t magic, version;
  int32_t lanes;       // W: lanes per utterance of the session (16 or 64)
  int32_t x_total;     // doubles of the saved LDS image (tree_core.h X_TOTAL)
  int32_t lane_bytes;  // sizeof(Lane<W>)
  int32_t latched;     // 1: the frame part is the voice's latched frame; 0: its next frame only latches
  uint32_t seed;       // what the saved voice was seeded with (informational; 0: not known)
  uint32_t reserved;   // 0
  double sampling_rate_hz;
  afs_options options;
  uint8_t pad[8];      // 0
};
static_assert(sizeof(VoiceStateHeader) == 96 && sizeof(VoiceStateHeader) % 16 == 0, "the header is six 16-byte vectors");

constexpr int VOICE_STATE_PARTS = 3;  // lanes, LDS image, latched frame

AFS_VS_HD inline int64_t voice_state_pad16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// Where the parts of a record lie, and how far apart the same part of two neighbouring voices lies in
// the session's buffer (the latched frame is pair[u][0] of afs_frame pair[B][2]).
struct VoiceStateLayout {
  int64_t bytes[VOICE_STATE_PARTS];   // of a part, as the session holds it
  int64_t offset[VOICE_STATE_PARTS];  // of a part in the record (a multiple of 16)
  int64_t stride[VOICE_STATE_PARTS];  // bytes from voice u's part to voice u + 1's in the session's buffer
  int64_t record_bytes;               // a multiple of 16
};

AFS_VS_HD inline VoiceStateLayout voice_state_layout(int lanes, int64_t lane_bytes, int64_t x_total, int64_t frame_bytes) {
  VoiceStateLayout L{};
  L.bytes[0] = (int64_t)lanes * lane_bytes, L.stride[0] = L.bytes[0];
  L.bytes[1] = x_total * (int64_t)sizeof(double), L.stride[1] = L.bytes[1];
  L.bytes[2] = frame_bytes, L.stride[2] = 2 * frame_bytes;
  int64_t at = (int64_t)sizeof(VoiceStateHeader);
  for (int p = 0; p < VOICE_STATE_PARTS; ++p) {
    L.offset[p] = at;
    at += voice_state_pad16(L.bytes[p]);
  }
  L.record_bytes = at;
  return L;
}

// 16-byte vectors of a record's payload (everything behind the header)
AFS_VS_HD inline int64_t voice_state_payload_vecs(const VoiceStateLayout &L) {
  return (L.record_bytes - (int64_t)sizeof(VoiceStateHeader)) / 16;
}

// Payload vector v of a record of voice u: its byte offset in the record, the part it belongs to and its
// byte offset in that part's buffer of the session.  part < 0: a vector of padding (none while every part
// is whole vectors, which the kernels require).
struct VoiceStateVec {
  int part;
  int64_t record_off, session_off;
};
AFS_VS_HD inline VoiceStateVec voice_state_vec(const VoiceStateLayout &L, int64_t v, int64_t u) {
  VoiceStateVec r;
  r.record_off = (int64_t)sizeof(VoiceStateHeader) + 16 * v;
  int p = 0;
  while (p + 1 < VOICE_STATE_PARTS && r.record_off >= L.offset[p + 1]) ++p;
  const int64_t in_part = r.record_off - L.offset[p];
  r.part = in_part + 16 <= L.bytes[p] ? p : -1;
  r.session_off = u * L.stride[p] + in_part;
  return r;
}

// ---- the header (host) ----

inline bool voice_state_options_equal(const afs_options &a, const afs_options &b) {
  return a.turbulence_losses == b.turbulence_losses && a.soft_walls == b.soft_walls &&
         a.generate_noise_sources == b.generate_noise_sources && a.radiation_from_skin == b.radiation_from_skin &&
         a.piriform_fossa == b.piriform_fossa && a.inner_length_corrections == b.inner_length_corrections &&
         a.transvelar_coupling == b.transvelar_coupling && a.glottis_loss == b.glottis_loss &&
         a.glottis_model == b.glottis_model && a.flow_separation_area_ratio == b.flow_separation_area_ratio;
}

// the header of a voice of a session of `lanes` lanes on a context of this rate and these options; every
// byte defined (the options field by field: the struct's own padding stays 0)
inline VoiceStateHeader voice_state_header(int lanes, int64_t lane_bytes, int64_t x_total, double rate,
                                           const afs_options &o, bool latched, uint32_t seed) {
  VoiceStateHeader h;
  std::memset(&h, 0, sizeof h);
  h.magic = VOICE_STATE_MAGIC, h.version = VOICE_STATE_VERSION;
  h.lanes = lanes, h.x_total = (int32_t)x_total, h.lane_bytes = (int32_t)lane_bytes;
  h.latched = latched ? 1 : 0, h.seed = seed;
  h.sampling_rate_hz = rate;
  h.options.turbulence_losses = o.turbulence_losses, h.options.soft_walls = o.soft_walls;
  h.options.generate_noise_sources = o.generate_noise_sources, h.options.radiation_from_skin = o.radiation_from_skin;
  h.options.piriform_fossa = o.piriform_fossa, h.options.inner_length_corrections = o.inner_length_corrections;
  h.options.transvelar_coupling = o.transvelar_coupling, h.options.glottis_loss = o.glottis_loss;
  h.options.glottis_model = o.glottis_model, h.options.flow_separation_area_ratio = o.flow_separation_area_ratio;
  return h;
}

// Why a record's header does not fit a session whose own records carry `want` (null: it fits).  The
// latched flag and the seed are the voice's, not the session's.
inline const char *voice_state_mismatch(const VoiceStateHeader &h, const VoiceStateHeader &want) {
  if (h.magic != want.magic) return "not a voice record (magic)";
  if (h.version != want.version) return "another layout version";
  if (h.lanes != want.lanes) return "another lane width";
  if (h.x_total != want.x_total || h.lane_bytes != want.lane_bytes) return "another state size (X_TOTAL, sizeof(Lane))";
  if (!(h.sampling_rate_hz == want.sampling_rate_hz)) return "another sampling rate";
  if (!voice_state_options_equal(h.options, want.options)) return "other options";
  if (h.latched != 0 && h.latched != 1) return "a latched flag outside 0, 1";
  return nullptr;
}

}  // namespace afs
