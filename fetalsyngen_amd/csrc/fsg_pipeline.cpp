// fsg_pipeline.cpp -- the fused per-sample launch sequence as ONE native call.
//
// Host-side only (no kernels here): enqueues, on the caller's stream, exactly the sequence
// `FetalSynthGen.sample` of the reference walks through (generator/model.py:231-276: generate -> augment),
// using the entry points declared in include/fsg_hip.h.  It exists because at ~30 us per kernel the Python
// interpreter between launches costs as much as the kernels; semantics and results are those of calling the
// entry points one by one (tests/test_hip_parity.py::test_native_pipeline_equals_stagewise).
#include <hip/hip_runtime.h>
#include <cstddef>
#include "../../include/fsg_hip.h"

// The one-launch head with the look-ahead's draw job beside it (fsg_deform.hip; not part of the public header): the public
// fsg_sample_head_* entry points plus (drawk, draw_blocks), and the form without a GMM job (fsg_sample_image::prior_in).
extern "C" int fsg_internal_head_no_gmm(size_t n, const fsg_deform* d, const fsg_epilogue* epi, float* rows, int row_stride,
                                        int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream);
extern "C" int fsg_internal_head_f32(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                                     const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                                     uint64_t stream_id, float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                                     int row_stride, int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream);
extern "C" int fsg_internal_head_codes_f32(const uint16_t* codes, const uint8_t* tuples, int ntuples, int stride,
                                           const int32_t sel[4], size_t n, const float* mus, const float* sigmas, int ntab,
                                           uint64_t seed, uint64_t stream_id, float* out, const fsg_deform* d,
                                           const fsg_epilogue* epi, float* rows, int row_stride, int32_t* mm3, const void* drawk,
                                           unsigned draw_blocks, void* stream);


extern int g_tuning_flags;

// Kept for the ABI (include/fsg_hip.h): the library owns no streams or events, so there is nothing to release.
extern "C" int fsg_pipeline_teardown(void) { return 0; }

#define FSG_TRY(expr)        \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != 0) return rc_; \
  } while (0)
#define FSG_HIP(expr)                          \
  do {                                         \
    hipError_t e_ = (expr);                    \
    if (e_ != hipSuccess) return (int)e_;      \
  } while (0)

extern "C" int fsg_sample_run(const fsg_sample_plan* p, void* stream) { return fsg_sample_run_image(p, nullptr, stream); }

extern "C" int fsg_internal_sample_run(const fsg_sample_plan* p, const fsg_sample_image* im, int floormin_settled, void* stream);
extern "C" int fsg_sample_run_image(const fsg_sample_plan* p, const fsg_sample_image* im, void* stream) {
  return fsg_internal_sample_run(p, im, 0, stream);
}

// floormin_settled (fsg_keyed_sample_run's host verdict, fsg_keyed.hip): the caller has PROVED that the faces job of the fused
// head leaves every floor(min) key below key(1.0), so the conditional full pass behind it would return at once -- it is not
// launched (FSG_TUNE_NO_FLOORMIN_SKIP: launched all the same).  0: no such proof, the pass runs as ever.
extern "C" int fsg_internal_sample_run(const fsg_sample_plan* p, const fsg_sample_image* im, int floormin_settled, void* stream) {
  if (!p || !p->out || !p->ws0 || !p->ws1 || !p->mm8) return FSG_E_BADARG;
  const int n0 = p->shape[0], n1 = p->shape[1], n2 = p->shape[2];
  if (n0 <= 0 || n1 <= 0 || n2 <= 0) return FSG_E_BADARG;
  const size_t n = (size_t)n0 * n1 * n2;
  if (n > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  const float* const image_in = im ? im->image_in : nullptr;
  float* const image_out = im ? im->image_out : nullptr;
  if (image_in && !image_out) return FSG_E_BADARG;
  const float* const prior = im ? im->prior_in : nullptr;  // given intensities instead of the GMM draw
  hipStream_t st = (hipStream_t)stream;
  int rode = 0;  // look-ahead jobs that really went out (fsg_sample_plan::rode)
  if (p->rode) *p->rode = 0;

  // stage trace (measurement only): an event behind every launch, see fsg_sample_plan::trace_events
  int ntrace = p->trace_start > 0 ? p->trace_start : 0;
  auto mark = [&](int id) -> int {
    if (!p->trace_events || !p->trace_ids || ntrace >= p->trace_cap) return 0;
    hipError_t e = hipEventRecord((hipEvent_t)p->trace_events[ntrace], st);
    if (e != hipSuccess) return (int)e;
    p->trace_ids[ntrace++] = id;
    p->trace_ids[p->trace_cap] = ntrace;
    return 0;
  };
  FSG_TRY(mark(p->trace_start > 0 ? p->trace_first_id : FSG_ST_BEGIN));

  const bool has_gamma = p->epi.gamma > 0.f, has_bias = p->epi.bias != nullptr;
  bool head_done = false;
  fsg_deform dh = p->deform;
  const int need_h = 3 * dh.field_dims[2] + (has_bias ? p->epi.bias_dims[2] : 0);
  const bool fused_head = p->deform_active && p->mm8_preset && p->ws_rows && !(g_tuning_flags & FSG_TUNE_SPLIT_HEAD) &&
                          need_h > 0 && need_h <= p->row_stride;
  if (p->arena_host) {  // the sample's parameter block, copied on the launch stream before its first kernel
    if (!p->arena_dev || (p->arena_bytes & 15)) return FSG_E_BADARG;
    FSG_TRY(fsg_copy_bytes(p->arena_dev, p->arena_host, (size_t)p->arena_bytes, stream));
    FSG_TRY(mark(FSG_ST_UPLOAD));
  }
  int head_rc = 0;
  const void* const ride = p->ride_draw && p->ride_draw_blocks ? p->ride_draw : nullptr;  // + the next sample's draw job
  const unsigned ride_blocks = ride ? p->ride_draw_blocks : 0u;
  if (fused_head) {
    // K1 + per-row coarse values + six-face minimum in one launch (keys arrive initialised with the parameters)
    dh.rows = nullptr;
    dh.row_stride = 0;
    head_rc = FSG_E_ALIGN;
    if (prior)  // rows + faces; the GMM job has nothing to draw
      head_rc = fsg_internal_head_no_gmm(n, &dh, &p->epi, p->ws_rows, p->row_stride, p->mm8, ride, ride_blocks, stream);
    else if (p->label_codes && p->code_tuples && !p->gmm_noise && !(g_tuning_flags & FSG_TUNE_NO_SEED_CODES))  // 6 instead of 8 B/voxel
      head_rc = fsg_internal_head_codes_f32(p->label_codes, p->code_tuples, p->code_ntuples, p->code_stride, p->code_sel, n, p->mus,
                                            p->sigmas, p->ntab, p->gmm_seed, p->gmm_stream, p->ws0, &dh, &p->epi, p->ws_rows,
                                            p->row_stride, p->mm8, ride, ride_blocks, stream);
    if (!prior && (head_rc == FSG_E_ALIGN || head_rc == FSG_E_TOOBIG))  // no codes, or outside their domain: the four label volumes
      head_rc = fsg_internal_head_f32(p->label_parts[0], p->label_parts[1], p->label_parts[2], p->label_parts[3], n, p->mus,
                                      p->sigmas, p->ntab, p->gmm_noise, p->gmm_seed, p->gmm_stream, p->ws0, &dh, &p->epi,
                                      p->ws_rows, p->row_stride, p->mm8, ride, ride_blocks, stream);
    if (head_rc == 0) head_done = true;
    if (head_done && ride) rode |= 1;
    if (head_done) FSG_TRY(mark(FSG_ST_HEAD));
  }
  if (head_rc != 0 && head_rc != FSG_E_TOOBIG && head_rc != FSG_E_ALIGN) return head_rc;
  // K1: GMM draw -> ws0; the same launch resets every min/max key of the sample (unless they arrived initialised):
  // [min x,y,z | zoom min] [zoom max | 3 unused]
  if (!head_done && prior) {
    if (!p->mm8_preset) FSG_TRY(fsg_minmax_init(p->mm8, 4, 4, stream));
  } else if (!head_done)
    FSG_TRY(fsg_gmm_sample_u8x4_mm(p->label_parts[0], p->label_parts[1], p->label_parts[2], p->label_parts[3], n,
                                   p->mus, p->sigmas, p->ntab, p->gmm_noise, p->gmm_seed, p->gmm_stream, p->ws0,
                                   p->mm8_preset ? nullptr : p->mm8, 4, 4, stream));
  if (!head_done && !prior) FSG_TRY(mark(FSG_ST_GMM));
  // `cur` holds the volume so far, `other` receives the next stage.  The prior is read-only: it starts as `cur` and leaves the
  // rotation at the first stage that consumes it.
  float* cur = prior ? const_cast<float*>(prior) : p->ws0;
  float* other = prior ? p->ws0 : p->ws1;
  auto rotate = [&]() {
    float* t = cur;
    cur = other;
    other = t == prior ? p->ws1 : t;
  };

  if (p->deform_active) {
    // K2/K3: coarse rows, floor(min) margins; K4(+K5): fused warp of the image and the labels -> ws1
    if (!p->seg_in || (!p->seg_out && !p->seg_out_u8) || (p->seg_out_u8 && !p->seg_in_u8)) return FSG_E_BADARG;
    fsg_deform d = p->deform;
    const int need = 3 * d.field_dims[2] + (has_bias ? p->epi.bias_dims[2] : 0);
    if (head_done) {
      d.rows = p->ws_rows;
      d.row_stride = p->row_stride;
      if (!floormin_settled || (g_tuning_flags & FSG_TUNE_NO_FLOORMIN_SKIP)) {
        FSG_TRY(fsg_coords_floormin_rest_f32(&d, p->mm8, stream));
        FSG_TRY(mark(FSG_ST_FLOORMIN));
      }
    } else {
      if (p->ws_rows && need > 0 && need <= p->row_stride) {
        d.rows = nullptr;
        d.row_stride = 0;
        FSG_TRY(fsg_deform_rows_f32(&d, &p->epi, p->ws_rows, p->row_stride, stream));
        FSG_TRY(mark(FSG_ST_ROWS));
        d.rows = p->ws_rows;
        d.row_stride = p->row_stride;
      } else {
        d.rows = nullptr;
        d.row_stride = 0;
      }
      int rc = fsg_coords_floormin_f32(&d, p->mm8, stream);
      if (rc == FSG_E_TOOBIG) {  // coarse grid beyond the row kernels: exact min/max (6 keys) into a side buffer
        return FSG_E_TOOBIG;     // the Python orchestration handles this rare configuration stage by stage
      }
      FSG_TRY(rc);
      FSG_TRY(mark(FSG_ST_FLOORMIN));
    }
    int rw = FSG_E_ALIGN;
    bool image_done = false;
    if (image_in) {  // the real image in the same launch (same label sources as below); FSG_E_ALIGN: the two-launch form
      const bool in_u8 = p->seg_out_u8 || p->seg_in_u8;
      const void* src_nn = in_u8 ? (const void*)p->seg_in_u8 : (const void*)p->seg_in;
      void* out_nn = p->seg_out_u8 ? (void*)p->seg_out_u8 : (void*)p->seg_out;
      rw = fsg_warp_dual_f32(&d, p->mm8, cur, other, image_in, image_out, n, src_nn, out_nn, in_u8 ? FSG_LABEL_U8 : FSG_LABEL_F32,
                             p->seg_out_u8 ? FSG_LABEL_U8 : FSG_LABEL_F32, &p->epi, stream);
      image_done = rw == 0;
    }
    if (image_done) {
    } else if (p->seg_out_u8) {  // uint8 labels in and out (same values: labels are integers 0..255)
      rw = fsg_warp_f32_u8(&d, p->mm8, cur, other, p->seg_in_u8, p->seg_out_u8, &p->epi, stream);
    } else {
      rw = FSG_E_ALIGN;
      if (p->seg_in_u8)  // uint8 copy of the labels: 1 B/voxel gathered instead of 4 (same output)
        rw = fsg_warp_f32_u8_to_f32(&d, p->mm8, cur, other, p->seg_in_u8, p->seg_out, &p->epi, stream);
      if (rw == FSG_E_ALIGN) rw = fsg_warp_f32(&d, p->mm8, cur, other, p->seg_in, p->seg_out, &p->epi, stream);
    }
    FSG_TRY(rw);
    FSG_TRY(mark(FSG_ST_WARP));
    if (image_in && !image_done) {
      const fsg_epilogue none = {};
      FSG_TRY(fsg_warp_f32(&d, p->mm8, image_in, image_out, nullptr, nullptr, &none, stream));
      FSG_TRY(mark(FSG_ST_WARP));
    }
    rotate();
  } else {
    if (has_gamma) {
      FSG_TRY(fsg_gamma_f32(cur, n, p->epi.gamma, other, stream));
      FSG_TRY(mark(FSG_ST_POINTWISE));
      rotate();
    }
    if (has_bias) {
      FSG_TRY(fsg_bias_mul_f32(cur, n0, n1, n2, p->epi.bias, p->epi.bias_dims[0], p->epi.bias_dims[1],
                               p->epi.bias_dims[2], p->epi.bx, p->epi.by, p->epi.bz, other, stream));
      FSG_TRY(mark(FSG_ST_POINTWISE));
      rotate();
    }
  }

  if (p->resample_active) {
    if (!p->ws_low) return FSG_E_BADARG;
    const int m0 = p->low_shape[0], m1 = p->low_shape[1], m2 = p->low_shape[2];
    // K6 + K7 + K8 as the fused pair (csrc/fsg_blur_rs.hip): blur and down-sampling of an axis in one operator, the blurred
    // full-resolution volume never exists.  Bracketed by the caller's HIP events like the unfused blur below.
    const bool fused_rs = fsg_blur_resample_supported(n0, n1, n2, m0, m1, m2, p->blur_ntaps[0], p->blur_ntaps[1], p->blur_ntaps[2]);
    if (fused_rs) {
      if (p->ev_blur_begin) FSG_HIP(hipEventRecord((hipEvent_t)p->ev_blur_begin, st));
      FSG_TRY(fsg_blur_resample_x_f32(cur, n0, n1, n2, p->rs_tab[0], m0, p->blur_taps[0], p->blur_ntaps[0], other, stream));
      FSG_TRY(mark(FSG_ST_BLUR_RS_X));
      FSG_TRY(fsg_blur_resample_yz_noise_f32(other, m0, n1, n2, p->rs_tab[1], p->rs_tab[2], m1, m2, p->blur_taps[1],
                                             p->blur_ntaps[1], p->blur_taps[2], p->blur_ntaps[2], p->noise_mode, p->noise,
                                             p->noise_seed, p->noise_stream, p->noise_std, p->ws_low, stream));
      FSG_TRY(mark(FSG_ST_BLUR_RS_YZ));
      if (p->ev_blur_end) FSG_HIP(hipEventRecord((hipEvent_t)p->ev_blur_end, st));
    } else {
    // K6: separable blur, x then y then z (optionally bracketed by the caller's HIP events: bench.py's live
    // measurement of the graded kernel on the launch stream)
    if (p->ev_blur_begin) FSG_HIP(hipEventRecord((hipEvent_t)p->ev_blur_begin, st));
    for (int axis = 0; axis < 3; ++axis) {
      const int nt = p->blur_ntaps[axis];
      if (nt <= 0) continue;
      if (axis == 1 && p->blur_ntaps[2] > 0 && !(g_tuning_flags & FSG_TUNE_NO_BLUR_FUSE)) {
        // y and z passes in one launch (intermediate in LDS); bit-identical to the two single-axis launches
        int rf = fsg_blur_yz_taps_host_f32(cur, other, n0, n1, n2, p->blur_taps[1], nt, p->blur_taps[2], p->blur_ntaps[2],
                                           stream);
        if (rf == 0) {
          FSG_TRY(mark(FSG_ST_BLUR_YZ));
          rotate();
          break;
        }
        if (rf != FSG_E_ALIGN) return rf;
      }
      int rc = fsg_blur_axis_taps_host_f32(cur, other, n0, n1, n2, axis, p->blur_taps[axis], nt, stream);
      if (rc == FSG_E_ALIGN) return FSG_E_ALIGN;  // shape outside the tuned kernels: stage-by-stage path
      FSG_TRY(rc);
      FSG_TRY(mark(FSG_ST_BLUR_X + axis));
      rotate();
    }
    if (p->ev_blur_end) FSG_HIP(hipEventRecord((hipEvent_t)p->ev_blur_end, st));
    // K7+K8: resample + noise -> low
    FSG_TRY(fsg_resample_noise_f32(cur, n0, n1, n2, p->rs_tab[0], p->rs_tab[1], p->rs_tab[2], p->ws_low, m0, m1, m2,
                                   p->noise_mode, p->noise, p->noise_seed, p->noise_stream, p->noise_std, stream));
    FSG_TRY(mark(FSG_ST_K7));
    }
    // K9 (+K10): min/max of the zoom-back, then zoom-back + normalise -> out
    if (p->mm_slots && p->mm_nslots >= 2 && p->mm_nslots <= 64) {  // keys sharded over slots: no contended address
      FSG_TRY(fsg_zoom3d_minmax_sharded_f32(p->ws_low, m0, m1, m2, p->back_tab[0], p->back_tab[1], p->back_tab[2], n0, n1,
                                            n2, p->mm_slots, p->mm_nslots, stream));
      FSG_TRY(mark(FSG_ST_K9A));
      FSG_TRY(fsg_zoom3d_normalise_sharded_f32(p->ws_low, m0, m1, m2, p->back_tab[0], p->back_tab[1], p->back_tab[2], p->out,
                                               n0, n1, n2, p->mm_slots, p->mm_nslots, p->scale01 ? 1 : 0, stream));
      FSG_TRY(mark(FSG_ST_K9B));
      if (p->rode) *p->rode = rode;
      return 0;
    }
    FSG_TRY(fsg_zoom3d_minmax_f32(p->ws_low, m0, m1, m2, p->back_tab[0], p->back_tab[1], p->back_tab[2], n0, n1, n2,
                                  p->mm8 + 3, stream));
    FSG_TRY(mark(FSG_ST_K9A));
    FSG_TRY(fsg_zoom3d_normalise_f32(p->ws_low, m0, m1, m2, p->back_tab[0], p->back_tab[1], p->back_tab[2], p->out, n0,
                                     n1, n2, p->mm8 + 3, p->scale01 ? 1 : 0, stream));
    FSG_TRY(mark(FSG_ST_K9B));
    if (p->rode) *p->rode = rode;
    return 0;
  }

  // no resampling: noise at full resolution, optional [0,1] scaling
  if (p->noise_mode != 0) {
    float* dst = p->scale01 ? other : p->out;
    FSG_TRY(fsg_add_noise_f32(cur, n, p->noise_mode == 1 ? p->noise : nullptr, p->noise_seed, p->noise_stream,
                              p->noise_std, dst, stream));
    cur = dst;
  }
  if (p->scale01) {
    FSG_TRY(fsg_reduce_minmax_f32(cur, n, p->mm8 + 3, stream));
    FSG_TRY(fsg_scale_f32(cur, n, p->mm8 + 3, 1, p->out, stream));
  } else if (cur != p->out) {
    hipError_t e = hipMemcpyAsync(p->out, cur, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  if (p->rode) *p->rode = rode;
  return 0;
}

extern "C" int64_t fsg_sample_plan_layout(int which) {
  switch (which) {
    case FSG_SIZEOF_SAMPLE_PLAN: return (int64_t)sizeof(fsg_sample_plan);
    case FSG_SIZEOF_TAP: return (int64_t)sizeof(fsg_tap);
    case FSG_SIZEOF_DEFORM: return (int64_t)sizeof(fsg_deform);
    case FSG_SIZEOF_EPILOGUE: return (int64_t)sizeof(fsg_epilogue);
    case FSG_SIZEOF_KEYED_CONFIG: return (int64_t)sizeof(fsg_keyed_config);
    case FSG_SIZEOF_KEYED_DRAWS: return (int64_t)sizeof(fsg_keyed_draws);
    case 1: return (int64_t)offsetof(fsg_sample_plan, blur_taps);
    case 2: return (int64_t)offsetof(fsg_sample_plan, out);
    case 3: return (int64_t)offsetof(fsg_sample_plan, seg_in_u8);
    case 4: return (int64_t)offsetof(fsg_sample_plan, ws_seq);
    case 5: return (int64_t)offsetof(fsg_sample_plan, code_sel);
    case FSG_SIZEOF_SAMPLE_IMAGE: return (int64_t)sizeof(fsg_sample_image);
    case FSG_SIZEOF_KEYED_OVERRIDES: return (int64_t)sizeof(fsg_keyed_overrides);
    default: return -1;
  }
}

// The plan from two flat arrays instead of ~60 field writes through an FFI (the Python mirror spends 41 us filling the
// struct field by field through ctypes: profiles/r02_c_host_phases.txt).  Index layout: FSG_PLAN_I_* / FSG_PLAN_F_* in
// include/fsg_hip.h.  `taps`: 3 x FSG_PLAN_TAPS_STRIDE floats, row a = the Gaussian taps of axis a.
extern "C" int fsg_sample_plan_pack(fsg_sample_plan* p, const int64_t* iv, int niv, const double* fv, int nfv,
                                    const float* taps) {
  if (!p || !iv || !fv || niv < FSG_PLAN_I_COUNT || nfv < FSG_PLAN_F_COUNT) return FSG_E_BADARG;
  fsg_sample_plan q = {};
  for (int a = 0; a < 3; ++a) q.shape[a] = (int32_t)iv[FSG_PLAN_I_SHAPE + a];
  for (int a = 0; a < 4; ++a) q.label_parts[a] = (const uint8_t*)(uintptr_t)iv[FSG_PLAN_I_LABEL_PARTS + a];
  q.mus = (const float*)(uintptr_t)iv[FSG_PLAN_I_MUS];
  q.sigmas = (const float*)(uintptr_t)iv[FSG_PLAN_I_SIGMAS];
  q.ntab = (int32_t)iv[FSG_PLAN_I_NTAB];
  q.gmm_noise = (const float*)(uintptr_t)iv[FSG_PLAN_I_GMM_NOISE];
  q.gmm_seed = (uint64_t)iv[FSG_PLAN_I_GMM_SEED];
  q.gmm_stream = (uint64_t)iv[FSG_PLAN_I_GMM_STREAM];
  q.deform_active = (int32_t)iv[FSG_PLAN_I_DEFORM_ACTIVE];
  if (q.deform_active) {
    for (int a = 0; a < 3; ++a) q.deform.shape[a] = q.shape[a];
    for (int a = 0; a < 9; ++a) q.deform.A[a] = (float)fv[FSG_PLAN_F_A + a];
    for (int a = 0; a < 3; ++a) {
      q.deform.centre[a] = (float)fv[FSG_PLAN_F_CENTRE + a];
      q.deform.c2[a] = (float)fv[FSG_PLAN_F_C2 + a];
      q.deform.field_dims[a] = (int32_t)iv[FSG_PLAN_I_FIELD_DIMS + a];
    }
    q.deform.flip = (int32_t)iv[FSG_PLAN_I_FLIP];
    q.deform.field = (const float*)(uintptr_t)iv[FSG_PLAN_I_FIELD];
    q.deform.tx = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_FIELD_TABS];
    q.deform.ty = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_FIELD_TABS + 1];
    q.deform.tz = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_FIELD_TABS + 2];
  }
  q.seg_in = (const float*)(uintptr_t)iv[FSG_PLAN_I_SEG_IN];
  q.seg_out = (float*)(uintptr_t)iv[FSG_PLAN_I_SEG_OUT];
  q.seg_in_u8 = (const uint8_t*)(uintptr_t)iv[FSG_PLAN_I_SEG_IN_U8];
  q.epi.gamma = (float)fv[FSG_PLAN_F_GAMMA];
  for (int a = 0; a < 3; ++a) q.epi.bias_dims[a] = (int32_t)iv[FSG_PLAN_I_BIAS_DIMS + a];
  q.epi.bias = (const float*)(uintptr_t)iv[FSG_PLAN_I_BIAS];
  q.epi.bx = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_BIAS_TABS];
  q.epi.by = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_BIAS_TABS + 1];
  q.epi.bz = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_BIAS_TABS + 2];
  q.resample_active = (int32_t)iv[FSG_PLAN_I_RESAMPLE_ACTIVE];
  for (int a = 0; a < 3; ++a) {
    q.low_shape[a] = (int32_t)iv[FSG_PLAN_I_LOW_SHAPE + a];
    q.rs_tab[a] = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_RS_TABS + a];
    q.back_tab[a] = (const fsg_tap*)(uintptr_t)iv[FSG_PLAN_I_BACK_TABS + a];
    const int nt = (int)iv[FSG_PLAN_I_BLUR_NTAPS + a];
    if (nt < 0 || nt > 129 || (nt > 0 && !taps)) return FSG_E_BADARG;
    q.blur_ntaps[a] = nt;
    for (int t = 0; t < nt; ++t) q.blur_taps[a][t] = taps[a * FSG_PLAN_TAPS_STRIDE + t];
  }
  q.noise_mode = (int32_t)iv[FSG_PLAN_I_NOISE_MODE];
  q.noise = (const float*)(uintptr_t)iv[FSG_PLAN_I_NOISE];
  q.noise_seed = (uint64_t)iv[FSG_PLAN_I_NOISE_SEED];
  q.noise_stream = (uint64_t)iv[FSG_PLAN_I_NOISE_STREAM];
  q.noise_std = (float)fv[FSG_PLAN_F_NOISE_STD];
  q.scale01 = (int32_t)iv[FSG_PLAN_I_SCALE01];
  q.ws0 = (float*)(uintptr_t)iv[FSG_PLAN_I_WS0];
  q.ws1 = (float*)(uintptr_t)iv[FSG_PLAN_I_WS1];
  q.ws_low = (float*)(uintptr_t)iv[FSG_PLAN_I_WS_LOW];
  q.ws_rows = (float*)(uintptr_t)iv[FSG_PLAN_I_WS_ROWS];
  q.row_stride = (int32_t)iv[FSG_PLAN_I_ROW_STRIDE];
  q.mm8 = (int32_t*)(uintptr_t)iv[FSG_PLAN_I_MM8];
  q.mm8_preset = (int32_t)iv[FSG_PLAN_I_MM8_PRESET];
  q.out = (float*)(uintptr_t)iv[FSG_PLAN_I_OUT];
  q.ev_blur_begin = (void*)(uintptr_t)iv[FSG_PLAN_I_EV_BEGIN];
  q.ev_blur_end = (void*)(uintptr_t)iv[FSG_PLAN_I_EV_END];
  q.mm_slots = (int32_t*)(uintptr_t)iv[FSG_PLAN_I_MM_SLOTS];
  q.mm_nslots = (int32_t)iv[FSG_PLAN_I_MM_NSLOTS];
  q.arena_host = (const void*)(uintptr_t)iv[FSG_PLAN_I_ARENA_HOST];
  q.arena_dev = (void*)(uintptr_t)iv[FSG_PLAN_I_ARENA_DEV];
  q.arena_bytes = (uint64_t)iv[FSG_PLAN_I_ARENA_BYTES];
  q.overlap = (int32_t)iv[FSG_PLAN_I_OVERLAP];  // retired fields: carried over, ignored by fsg_sample_run
  q.ws_seq = (uint64_t)iv[FSG_PLAN_I_WS_SEQ];
  q.seg_out_u8 = (uint8_t*)(uintptr_t)iv[FSG_PLAN_I_SEG_OUT_U8];
  q.trace_events = (void**)(uintptr_t)iv[FSG_PLAN_I_TRACE_EVENTS];
  q.trace_ids = (int32_t*)(uintptr_t)iv[FSG_PLAN_I_TRACE_IDS];
  q.trace_cap = (int32_t)iv[FSG_PLAN_I_TRACE_CAP];
  *p = q;
  return 0;
}

// pack + run in one call (what the Python mirror's fast path uses per sample)
extern "C" int fsg_sample_pack_run(const int64_t* iv, int niv, const double* fv, int nfv, const float* taps, void* stream) {
  fsg_sample_plan p;
  FSG_TRY(fsg_sample_plan_pack(&p, iv, niv, fv, nfv, taps));
  return fsg_sample_run(&p, stream);
}

// B samples with one native call (B volumes per call for DataLoader-style consumers).  Plan b is enqueued on
// streams[b % nstreams]; with nstreams > 1 consecutive samples overlap their kernel tails (the caller has ordered those
// streams behind the upload of the plans' parameters and joins them afterwards).  Results are those of B fsg_sample_run
// calls: the kernels, their arguments and their order per sample are the same.
extern "C" int fsg_sample_run_batch(const fsg_sample_plan* plans, int nplans, void* const* streams, int nstreams) {
  if (!plans || nplans < 0 || !streams || nstreams < 1) return FSG_E_BADARG;
  for (int b = 0; b < nplans; ++b) FSG_TRY(fsg_sample_run(&plans[b], streams[b % nstreams]));
  return 0;
}

// Thin hipEvent helpers so a ctypes caller can time sections of fsg_sample_run on the launch stream.
extern "C" void* fsg_event_create(void) {
  hipEvent_t e = nullptr;
  return hipEventCreate(&e) == hipSuccess ? (void*)e : nullptr;
}
extern "C" int fsg_event_record(void* e, void* stream) {
  return e ? (int)hipEventRecord((hipEvent_t)e, (hipStream_t)stream) : FSG_E_BADARG;
}
extern "C" int fsg_event_destroy(void* e) { return e ? (int)hipEventDestroy((hipEvent_t)e) : FSG_E_BADARG; }
extern "C" int fsg_event_elapsed_ms(void* begin, void* end, float* ms) {
  if (!begin || !end || !ms) return FSG_E_BADARG;
  hipError_t rc = hipEventSynchronize((hipEvent_t)end);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)begin, (hipEvent_t)end);
}
