// Selected-clip inference on several videos per forward (include/decafnet_hip_select_videos.h): the compaction and the gather of
// select.hip with a video per workgroup / per grid plane (the device code is the one body of select.h), and dcf_select_videos, the
// first call of the pattern for a whole forward: scores, gates and clip lists of every video.  The two forwards of the extension
// live in engine.hip beside the forwards they are a form of.
#include "../../include/decafnet_hip_select_videos.h"
#include "engine.h"
#include "select.h"

namespace dcf {

// what travels by value in the kernel argument: the first query row of every video (and the end of the last)
struct SelQueryOffsets { int q[DCF_MAX_VIDEOS + 1]; };

// workgroup v = k_select_clips on video v
__global__ __launch_bounds__(SEL_NT) void k_select_clips_videos(const float* __restrict__ gate, const uint8_t* __restrict__ masks, int T,
                                                                SelQueryOffsets qo, int* __restrict__ clips, int* __restrict__ pos,
                                                                int* __restrict__ counts) {
  const int v = blockIdx.x;
  const long long o = (long long)v * T;
  select_clips_body(gate + (long long)qo.q[v] * T, masks + o, T, qo.q[v + 1] - qo.q[v], clips + o, pos + o, counts + v);
}

struct GatherVideos {
  const void* X[DCF_MAX_VIDEOS];
  int first[DCF_MAX_VIDEOS + 1];
};
// blockIdx.z = the video; its tiles start at its own first row
template <typename E>
__global__ __launch_bounds__(GAT_NT) void k_gather_clip_rows_videos(GatherVideos gv, long long ldx, const int* __restrict__ clips, int T, int D,
                                                                    E* __restrict__ rows) {
  const int v = blockIdx.z;
  const int n = gv.first[v + 1] - gv.first[v], i0 = blockIdx.x * GAT_SIDE;
  if (i0 >= n) return;                              // (the grid is as wide as the longest list; the whole workgroup leaves)
  gather_clip_rows_tile<E>(static_cast<const E*>(gv.X[v]), ldx, clips + (long long)v * T, n, D, rows + (long long)gv.first[v] * D, i0,
                           blockIdx.y * GAT_SIDE);
}

static int launch_select_clips_videos(const char* who, const float* gate, const uint8_t* masks, int T, int nvid, const int32_t* nq_per_video,
                                      int32_t* clips, int32_t* pos, int32_t* counts, hipStream_t st) {
  DCF_CHECK(gate && masks && nq_per_video && clips && pos && counts, "%s: null argument", who);
  DCF_CHECK(T >= 1 && nvid >= 1 && nvid <= DCF_MAX_VIDEOS, "%s: T %d (>= 1), %d videos (1 .. %d)", who, T, nvid, DCF_MAX_VIDEOS);
  DCF_CHECK((reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(clips) | reinterpret_cast<uintptr_t>(pos) |
             reinterpret_cast<uintptr_t>(counts)) % 4 == 0, "%s: gate / clips / pos / counts not aligned to 4 bytes", who);
  SelQueryOffsets qo{};
  for (int v = 0; v < nvid; ++v) {
    DCF_CHECK(nq_per_video[v] >= 1 && nq_per_video[v] <= DCF_MAX_VIDEOS * 64, "%s: video %d has %d queries", who, v, (int)nq_per_video[v]);
    qo.q[v + 1] = qo.q[v] + nq_per_video[v];
  }
  ProfScope prof("select_clips_videos", st, 0.0, (4.0 * qo.q[nvid] + (1.0 + 8.0) * nvid) * (double)T);
  hipLaunchKernelGGL(k_select_clips_videos, dim3(nvid), dim3(SEL_NT), 0, st, gate, masks, T, qo, clips, pos, counts);
  DCF_HIP(hipGetLastError());
  return 0;
}

template <typename E>
static int launch_gather_videos(const char* who, const void* const* X, long long ldx, const int32_t* clips, int T, int nvid,
                                const int32_t* row_first, int D, void* rows, hipStream_t st) {
  DCF_CHECK(X && clips && row_first && rows, "%s: null argument", who);
  DCF_CHECK(nvid >= 1 && nvid <= DCF_MAX_VIDEOS, "%s: 1 .. %d videos per call (got %d)", who, DCF_MAX_VIDEOS, nvid);
  DCF_CHECK(T >= 1 && D >= 1 && ldx >= T, "%s: T %d, D %d (both >= 1), ldx %lld (>= T)", who, T, D, ldx);
  DCF_CHECK(reinterpret_cast<uintptr_t>(rows) % sizeof(E) == 0 && reinterpret_cast<uintptr_t>(clips) % 4 == 0,
            "%s: rows not aligned to its %d-byte elements, or clips not to 4 bytes", who, (int)sizeof(E));
  GatherVideos gv{};
  int widest = 0;
  DCF_CHECK(row_first[0] == 0, "%s: row_first[0] = %d, not 0", who, (int)row_first[0]);
  for (int v = 0; v < nvid; ++v) {
    const int n = row_first[v + 1] - row_first[v];
    DCF_CHECK(n >= 0 && n <= T, "%s: video %d has %d rows (0 .. T = %d)", who, v, n, T);
    DCF_CHECK(X[v] && reinterpret_cast<uintptr_t>(X[v]) % sizeof(E) == 0, "%s: X_cm[%d] is null or not aligned to its element", who, v);
    gv.X[v] = X[v]; gv.first[v] = row_first[v];
    widest = n > widest ? n : widest;
  }
  gv.first[nvid] = row_first[nvid];
  if (widest == 0) return 0;
  const long long gy = ((long long)D + GAT_SIDE - 1) / GAT_SIDE;
  DCF_CHECK(gy <= 65535, "%s: D %d exceeds one grid", who, D);
  ProfScope prof("gather_clip_rows_videos", st, 0.0, (2.0 * sizeof(E) * D + 4.0) * (double)row_first[nvid]);
  hipLaunchKernelGGL(k_gather_clip_rows_videos<E>, dim3((unsigned)((widest + GAT_SIDE - 1) / GAT_SIDE), (unsigned)gy, (unsigned)nvid),
                     dim3(GAT_NT), 0, st, gv, ldx, clips, T, D, static_cast<E*>(rows));
  DCF_HIP(hipGetLastError());
  return 0;
}

static int select_videos(dcf_model* m, const char* who, bool half, int nvid, const void* const* shallow, const uint8_t* const* vid_mask,
                         int64_t T64, const int32_t* nq_per_video, const float* const* text_cls, float* gate_out, float* correl_out,
                         int32_t* clips_out, int32_t* pos_out, int32_t* counts_out, hipStream_t st) {
  DCF_CHECK(m && shallow && vid_mask && nq_per_video && text_cls && gate_out && clips_out && pos_out && counts_out, "%s: null argument", who);
  DCF_CHECK(m->finalized, "%s: model not finalized", who);
  const dcf_config& c = m->cfg;
  DCF_CHECK(m->vid_w1, "%s: opt.model.sfonly reads no expert features: there is nothing to select", who);
  DCF_CHECK(vid_stride_of(c) == 1, "%s: vid_net.stride = %d: the externally gated forward takes vid_net.stride = 1", who, vid_stride_of(c));
  DCF_CHECK(nvid >= 1 && nvid <= DCF_MAX_VIDEOS, "%s: 1 .. %d videos per call (got %d)", who, DCF_MAX_VIDEOS, (int)nvid);
  DCF_CHECK(T64 >= 1 && T64 < (1ll << 24), "%s: T out of range", who);
  const int T = (int)T64, D = c.D;
  ScoreArgs sa{};
  int NQ = 0;
  for (int v = 0; v < nvid; ++v) {
    DCF_CHECK(shallow[v] && vid_mask[v] && text_cls[v] && nq_per_video[v] >= 1, "%s: video %d is incomplete", who, v);
    sa.shallow[v] = static_cast<const float*>(shallow[v]); sa.text_cls[v] = text_cls[v]; sa.nq[v] = nq_per_video[v]; sa.qoff[v] = NQ;
    NQ += nq_per_video[v];
    DCF_CHECK(NQ <= DCF_MAX_VIDEOS * 64, "%s: more than %d queries in all", who, DCF_MAX_VIDEOS * 64);
  }
  DCF_CHECK(c.sn >= 1 && (T + c.sn - 1) / c.sn <= 8192, "%s: more than 8192 pooling blocks (T=%d, sn=%d)", who, T, c.sn);
  DCF_CHECK((reinterpret_cast<uintptr_t>(gate_out) | reinterpret_cast<uintptr_t>(correl_out) | reinterpret_cast<uintptr_t>(clips_out) |
             reinterpret_cast<uintptr_t>(pos_out) | reinterpret_cast<uintptr_t>(counts_out)) % 4 == 0,
            "%s: gate_out / correl_out / clips_out / pos_out / counts_out not aligned to 4 bytes", who);
  // scratch: tn (NQ, D), partial [SCORE_SLICES][NQ + nvid][T], the scores where the caller does not want them, the masks side by
  // side and the gate kernel's second output (the clip masks of the forward, which makes them again)
  Arena ar{nullptr, 0, 0, true};
  auto carve = [&](Arena& a, float** tn, float** partial, float** correl, uint8_t** maskv, uint8_t** mask_q) {
    *tn = a.take<float>((size_t)NQ * D);
    *partial = a.take<float>((size_t)SCORE_SLICES * (NQ + nvid) * T);
    *correl = correl_out ? correl_out : a.take<float>((size_t)NQ * T);
    *maskv = a.take<uint8_t>((size_t)nvid * T);
    *mask_q = a.take<uint8_t>((size_t)NQ * T);
  };
  float *tn, *partial, *correl; uint8_t *maskv, *mask_q;
  carve(ar, &tn, &partial, &correl, &maskv, &mask_q);
  TRY(grow_half_ws(m, ar.off + 256, st));
  Arena aw{m->half_ws, 0, m->half_ws_bytes, false};
  carve(aw, &tn, &partial, &correl, &maskv, &mask_q);

  sa.nvid = nvid; sa.tn = tn; sa.partial = partial; sa.correl = correl; sa.D = D; sa.T = T; sa.NQ = NQ; sa.norm = c.norm;
  TRY(launch_sidekick(sa, st, half));
  TRY(launch_gather_masks(vid_mask, nvid, maskv, T, st));
  // the gate kernel names the video of a query in a nibble of vmap: 16 queries a launch
  for (int q0 = 0; q0 < NQ; q0 += 16) {
    const int B = NQ - q0 < 16 ? NQ - q0 : 16;
    unsigned long long vmap = 0;
    for (int i = 0, v = 0; i < B; ++i) {
      while (q0 + i >= sa.qoff[v] + sa.nq[v]) ++v;
      vmap |= (unsigned long long)v << (4 * i);
    }
    GateArgs ga{correl, maskv, gate_out + (size_t)q0 * T, mask_q + (size_t)q0 * T, T, B, q0, c.sn, c.msf, (double)c.sratio, vmap, nullptr, 0};
    TRY(launch_gate(ga, st));
  }
  return launch_select_clips_videos(who, gate_out, maskv, T, nvid, nq_per_video, clips_out, pos_out, counts_out, st);
}

}  // namespace dcf

extern "C" {

int dcf_select_videos_ext_version(void) { return DCF_SELECT_VIDEOS_EXT_VERSION; }

int dcf_op_select_clips_videos(const float* gate, const uint8_t* vid_masks, int32_t T, int32_t nvid, const int32_t* nq_per_video,
                               int32_t* clips, int32_t* pos, int32_t* counts, void* stream) {
  return dcf::launch_select_clips_videos("dcf_op_select_clips_videos", gate, vid_masks, T, nvid, nq_per_video, clips, pos, counts,
                                         (hipStream_t)stream);
}

int dcf_op_gather_clip_rows_videos(const float* const* X_cm, int64_t ldx, const int32_t* clips, int32_t T, int32_t nvid,
                                   const int32_t* row_first, int32_t D, float* rows, void* stream) {
  return dcf::launch_gather_videos<uint32_t>("dcf_op_gather_clip_rows_videos", reinterpret_cast<const void* const*>(X_cm), (long long)ldx,
                                             clips, T, nvid, row_first, D, rows, (hipStream_t)stream);
}

int dcf_op_gather_clip_rows_videos_h(const uint16_t* const* X_cm, int64_t ldx, const int32_t* clips, int32_t T, int32_t nvid,
                                     const int32_t* row_first, int32_t D, uint16_t* rows, void* stream) {
  return dcf::launch_gather_videos<uint16_t>("dcf_op_gather_clip_rows_videos_h", reinterpret_cast<const void* const*>(X_cm), (long long)ldx,
                                             clips, T, nvid, row_first, D, rows, (hipStream_t)stream);
}

int dcf_select_videos(dcf_model* m, int32_t nvid, const float* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                      const int32_t* nq_per_video, const float* const* text_cls, float* gate_out, float* correl_out, int32_t* clips_out,
                      int32_t* pos_out, int32_t* counts_out, void* stream) {
  return dcf::select_videos(m, "dcf_select_videos", false, nvid, reinterpret_cast<const void* const*>(shallow_vid), vid_mask, T, nq_per_video,
                            text_cls, gate_out, correl_out, clips_out, pos_out, counts_out, (hipStream_t)stream);
}

int dcf_select_videos_h(dcf_model* m, int32_t nvid, const uint16_t* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                        const int32_t* nq_per_video, const float* const* text_cls, float* gate_out, float* correl_out,
                        int32_t* clips_out, int32_t* pos_out, int32_t* counts_out, void* stream) {
  return dcf::select_videos(m, "dcf_select_videos_h", true, nvid, reinterpret_cast<const void* const*>(shallow_vid), vid_mask, T,
                            nq_per_video, text_cls, gate_out, correl_out, clips_out, pos_out, counts_out, (hipStream_t)stream);
}

}  // extern "C"
