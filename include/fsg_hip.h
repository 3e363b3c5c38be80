/*
 * fsg_hip.h -- C ABI of libfsg_hip.so: the MI355X (gfx950) kernels behind the
 * FetalSynthGen per-volume synthesis hot path.
 *
 * The reference (Medical-Image-Analysis-Laboratory/fetalsyngen) has no FFI on this path: it is
 * pure PyTorch tensor code.  The drop-in boundary is therefore the reference's Python class
 * surface (mirrored in fetalsyngen_amd/), and THIS header is what that mirror binds with ctypes
 * instead of calling ATen.  Each entry point names the reference code it replaces
 * (paths relative to /root/reference/fetalsyngen/).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all buffers;
 *   - volumes are C-contiguous (x, y, z) with z fastest, fp32 unless the name says otherwise;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous, no host sync inside,
 *     no allocation inside (safe to capture into a hipGraph);
 *   - return value: 0 = success, >0 = hipError_t of the launch, <0 = FSG_E_* argument error;
 *   - float arithmetic follows the reference's operation order with FMA contraction OFF in the
 *     coordinate / interpolation paths, so label volumes and sampling positions are bit-identical
 *     to the reference's CPU path on identical inputs.
 */
#ifndef FSG_HIP_H
#define FSG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_ABI_VERSION 8  /* 2: fsg_sample_plan grew (mm_slots .. seg_out_u8) after version 1 shipped; 3: label_codes .. code_sel, FSG_KEYED_I_CODES;
                              4: fsg_sample_image / fsg_sample_run_image, FSG_KEYED_I_IMAGE_IN .. PRIOR_IN, fsg_warp_dual_f32;
                              5: fsg_keyed_overrides / fsg_keyed_draw_with, fsg_keyed_draws grew (spacing3 .. sigmas_in),
                                 FSG_KEYED_I_OVERRIDES / BLOCK_BYTES;
                              6: fsg_voxel_pick_f32 / _u8, fsg_voxel_pick_ws_bytes;
                              7: fsg_slice_acq_adjoint_det_f32, fsg_slice_acq_adjoint_det_ws_bytes, FSG_SA_DET_FRAC_BITS / LIMB_BITS;
                              8: fsg_slice_acq_backward_f32, fsg_slice_acq_backward_ws_bytes; still 8 with
                                 fsg_slice_acq_adjoint_backward_f32 / _ws_bytes and with fsg_slice_acq_backward_det_f32 /
                                 _det_ws_bytes, and with fsg_axisangle2mat_f32 / fsg_mat2axisangle_f32 and their _backward_f32,
                                 and with fsg_cg_ws_bytes / fsg_cg_init_f32 / _q_f32 / _step_f32 / _dir_f32, and with
                                 fsg_svr_ws_bytes / fsg_svr_normal_f32 / fsg_svr_state_bytes / fsg_svr_update_f32, and with
                                 fsg_tk1_apply_f32, and with fsg_robust_ws_bytes / _state_bytes / _estep_f32 / _update_f32 /
                                 _weights_f32, and with fsg_imatch_ws_bytes / _state_bytes / _plane_bytes / _sums_f32 /
                                 _scale_f32 / _bias_f32 / _apply_f32, and with fsg_svr_compose_f32 / fsg_svr_group_reduce_f64:
                                 entries added, nothing older changed */

#define FSG_E_BADARG (-1)   /* null pointer / non-positive size / bad enum */
#define FSG_E_TOOBIG (-2)   /* size exceeds what the kernel indexes (2^31-1 voxels per volume) */
#define FSG_E_ALIGN  (-3)   /* pointer not aligned as the kernel requires */
#define FSG_E_NOTABLE (-4)  /* keyed mode: a tap table this sample needs was not registered (fsg_keyed_set_table) */

/* One output sample of a separable linear resample along one axis:
 * value = w_lo * src[lo] + w_hi * src[hi].  lo < 0 marks "outside" (result 0 for the voxel). */
typedef struct fsg_tap {
  int32_t lo;
  int32_t hi;
  float w_lo;
  float w_hi;
} fsg_tap;

/* Parameters of the spatial deformation (affine o nonlinear field), see fsg_coords_* / fsg_warp_*.
 * Passed BY POINTER from host memory; copied into the kernel arguments at launch. */
struct fsg_epilogue;

typedef struct fsg_deform {
  int32_t shape[3];      /* grid being generated == shape of the volumes being sampled            */
  float A[9];            /* row-major 3x3 affine, fp32 (affine_nonrigid.py:265-269)                */
  float centre[3];       /* (size-1)/2 of the configured size (affine_nonrigid.py:77-84)           */
  float c2[3];           /* rotation centre + shift, rounded to fp32 (affine_nonrigid.py:271-290)  */
  int32_t flip;          /* sample from the volume mirrored along axis 0 (affine_nonrigid.py:180)  */
  int32_t field_dims[3]; /* coarse displacement grid (s0,s1,s2); all 0 => no nonlinear field       */
  const float* field;    /* DEVICE (s0,s1,s2,3) fp32, channel-last, already scaled by nonlin_std   */
  const fsg_tap* tx;     /* DEVICE per-axis zoom tables coarse->shape, lengths shape[0..2]         */
  const fsg_tap* ty;
  const fsg_tap* tz;
  const float* rows;     /* DEVICE, optional (NULL = off): per-(x,y) coarse rows from fsg_deform_rows_f32 */
  int32_t row_stride;    /* floats per row in `rows`, >= 3*field_dims[2] (+ bias_dims[2] when fused)      */
} fsg_deform;

int fsg_abi_version(void);
const char* fsg_error_string(int code);

/* Process-wide tuning switches (tests use them to cross-check the tuned kernels against the plain
 * ones); returns the previous flags.  Results are within the documented tolerances either way. */
#define FSG_TUNE_GENERIC_WARP 1  /* per-voxel field evaluation instead of the row-wise LDS kernels */
#define FSG_TUNE_PRECISE_MATH 2  /* OCML powf/expf in the gamma/bias epilogue instead of v_log/v_exp; slice acquisition
                                    forward in the CUDA source's operation order instead of pair loads + lerps */
#define FSG_TUNE_GENERIC_ZOOM 4  /* per-voxel 8-tap zoom instead of the row-wise LDS kernels */
#define FSG_TUNE_NO_PREFETCH 8   /* row-wise zoom without the register-prefetch pipeline */
#define FSG_TUNE_NO_PATCH 32     /* row kernel (4 waves, own rows) instead of the 16-wave lockstep patch kernel */
#define FSG_TUNE_ROW_ZOOM 256    /* every zoom through the row-per-wave kernels (r01 default for K9) */
#define FSG_TUNE_TILE_ZOOM 512   /* every zoom through the tile kernel (default: only the noise epilogues) */
#define FSG_TUNE_NO_BLUR_FUSE 1024 /* blur: y and z passes as two launches */
#define FSG_TUNE_SA_DIRECT 128   /* slice-acquisition adjoint (interp_psf): direct global atomics, no LDS pre-summation */
#define FSG_TUNE_SPLIT_HEAD 2048 /* fsg_sample_run: GMM draw, per-row coarse values and six-face minimum as three launches */
#define FSG_TUNE_SLAB_ZOOM 8192 /* the slab zoom kernel also for the noise epilogues (default there: tile kernel) */
#define FSG_TUNE_NO_LEAN 4096  /* fused warp: the r01 patch kernel body instead of the lean body (fsg_warp_lean.hip) */
#define FSG_TUNE_NO_SEED_CODES 65536 /* A/B: the one-launch head reads the four label volumes even when the plan carries a code volume */
#define FSG_TUNE_SA_FWD_DIRECT 131072 /* slice-acquisition forward (linear PSF, no volume mask): direct global gathers for every slice */
#define FSG_TUNE_SA_FWD_PLATE 262144  /* ... the LDS plate kernel for every slice (default: chosen per slice by its orientation) */
#define FSG_TUNE_NO_BLUR_RS 16384 /* fsg_sample_run: blur x3 + K7 as separate launches instead of the fused blur+resample pair */
#define FSG_TUNE_NO_FLOORMIN_SKIP 524288 /* A/B: fsg_keyed_sample_run launches the conditional floor(min) pass even when the host has
                                          * proved it a no-op (same keys, same volumes) */
#define FSG_TUNE_NO_LABEL_BRICKS 1048576 /* A/B: the fused warp gathers every label even where a brick table is attached
                                          * (fsg_label_bricks_attach); same outputs bit for bit */
/* Bits 16, 64 and 32768 are retired (kernel variants measured slower and removed): ignored by fsg_set_tuning, never reuse them. */
int fsg_set_tuning(int flags);

/* ---- brick table of a uint8 label volume (what lets the fused warp skip label gathers) -------- */
/* One uint8 per 8x8x8 brick of the (n0,n1,n2) volume, partial bricks at the upper faces included, layout
 * [ceil(n0/8)][ceil(n1/8)][ceil(n2/8)]: the brick's label if all of its voxels are equal and that label is not 255,
 * else 255 ("mixed: gather"; a uniform brick of label 255 is mixed too, which stays correct).  Once per subject. */
#define FSG_LABEL_BRICKS_CAP 32768 /* bricks of the largest volume whose table the warp can use (256^3 has exactly as many) */
int fsg_label_bricks_u8(const uint8_t* labels_u8, int n0, int n1, int n2, uint8_t* map_out, void* stream);
/* Process-wide registry (a few entries, guarded by a mutex): the table `map` (DEVICE, 16-byte aligned, written by
 * fsg_label_bricks_u8) describes the (n0,n1,n2) uint8 volume at `labels_u8`.  The fused warp looks its label source up here
 * and uses the table when the registered shape equals the launch's and fsg_label_bricks_usable holds; the caller keeps
 * volume and table unchanged and alive until it detaches.  attach: 0, replacing an entry of the same volume; FSG_E_BADARG /
 * FSG_E_ALIGN on bad arguments; FSG_E_TOOBIG when the registry is full (the volume is then simply gathered).  detach: 1 if
 * there was an entry, else 0.  count: entries.  usable: 1 if a table of that shape is within the cap, else 0. */
int fsg_label_bricks_attach(const void* labels_u8, int n0, int n1, int n2, const void* map);
int fsg_label_bricks_detach(const void* labels_u8);
int fsg_label_bricks_count(void);
int fsg_label_bricks_usable(int n0, int n1, int n2);
/* Test hook: the cap fsg_label_bricks_usable applies, 1..FSG_LABEL_BRICKS_CAP (0 = back to FSG_LABEL_BRICKS_CAP).  Returns the
 * previous cap, or FSG_E_BADARG (setting unchanged). */
int fsg_label_bricks_set_cap(int cap);
/* Lockstep pacing of the lean warp kernel (speed only, results identical): 0 = chosen per launch, 5 = no barrier,
 * 6 = a barrier every second step, 7 = a barrier every step.  Returns the previous value, or FSG_E_BADARG (setting
 * unchanged) for any other value. */
int fsg_warp_set_variant(int variant);

/* ---- RNG ------------------------------------------------------------------------------------ */
/* Standard-normal field from Philox4x32-10 keyed (seed, stream_id), element e uses counter e/4,
 * lane e%4, Box-Muller.  Exactly the values the fused kernels below use when noise == NULL, so
 * tests can hand the same noise to the CPU oracle.  Replaces torch.randn(shape, device=...)
 * (rand_gmm.py:146-148, synthseg.py:230-232) in device-RNG mode. */
int fsg_randn_f32(float* out, size_t n, uint64_t seed, uint64_t stream_id, void* stream);

/* ---- K1: GMM intensity draw (generator/intensity/rand_gmm.py:146-149) ------------------------- */
/* out[v] = max(mus[l] + sigmas[l] * z[v], 0), l = labels[v] < ntab.
 * noise != NULL: z = noise (host-tape RNG mode); else z = Philox(seed, stream_id). */
int fsg_gmm_sample_u8(const uint8_t* labels, size_t n, const float* mus, const float* sigmas, int ntab,
                      const float* noise, uint64_t seed, uint64_t stream_id, float* out, void* stream);
int fsg_gmm_sample_i64(const int64_t* labels, size_t n, const float* mus, const float* sigmas, int ntab,
                       const float* noise, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* Same with the seed map given as the per-meta-label volumes load_seeds would sum (rand_gmm.py:90-99):
 * label = l0 + l1 + l2 + l3 formed on the fly (l1..l3 may be NULL).  Pointers 4-byte aligned, out 16-byte. */
int fsg_gmm_sample_u8x4(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                        const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                        uint64_t stream_id, float* out, void* stream);
/* Same, and additionally resets `nmin` + `nmax` min/max keys at `mm` (as fsg_minmax_init would): the GMM draw is
 * the first kernel of a sample, folding the reset into it saves a launch.  mm may be NULL. */
int fsg_gmm_sample_u8x4_mm(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                           const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                           uint64_t stream_id, float* out, int32_t* mm, int nmin, int nmax, void* stream);

/* Per-label count / sum / sum of squares of `values` (wave-level reductions); accumulates into the
 * caller-zeroed outputs.  Used to validate device-RNG GMM draws against mus/sigmas. */
int fsg_label_stats_u8(const uint8_t* labels, const float* values, size_t n, int nlabels,
                       unsigned long long* count, double* sum, double* sumsq, void* stream);

/* ---- separable linear zoom (utils/generation.py:310-397 myzoom_torch) -------------------------- */
/* src (sx,sy,sz,nch) -> dst (dx,dy,dz,nch), per-axis tables of lengths dx,dy,dz.  x, then y, then z,
 * each step w_lo*a + w_hi*b in fp32 without FMA.  Also the axis-aligned trilinear resample of
 * synthseg.py:87-104 (tables built from the float64 positions; lo<0 => 0). */
int fsg_zoom3d_f32(const float* src, int sx, int sy, int sz, int nch, const fsg_tap* tx, const fsg_tap* ty,
                   const fsg_tap* tz, float* dst, int dx, int dy, int dz, void* stream);

/* K7+K8 fused (synthseg.py:104 + :230-233): dst = max(zoom(src) + noise_std * z, 0); z as in K1.
 * noise_mode 0: no noise (dst = zoom(src)); 1: noise pointer; 2: Philox(seed, stream_id). */
int fsg_resample_noise_f32(const float* src, int sx, int sy, int sz, const fsg_tap* tx, const fsg_tap* ty,
                           const fsg_tap* tz, float* dst, int dx, int dy, int dz, int noise_mode,
                           const float* noise, uint64_t seed, uint64_t stream_id, float noise_std,
                           void* stream);

/* Tile shape of the zoom kernels: output y rows per workgroup (1..64, default 16) and the LDS floats reserved for the
 * x-blended source-row window (256..16000, default 12288); a tile whose window does not fit is evaluated without staging.
 * FSG_E_BADARG (setting unchanged) outside those ranges. */
int fsg_zoom_set_tuning(int y_rows, int cap_floats);
/* K9 pass A (synthseg.py:111-112): min and max of zoom(src) without storing it; mm[0]=min, mm[1]=max as
 * order-preserving int32 keys (see fsg_minmax_init).  An outside output (lo < 0 on any axis) counts as the +0.0 that
 * fsg_zoom3d_f32 stores there.  NaN outputs are ignored (all NaN: the keys are left as they were); -0.0 orders below +0.0. */
int fsg_zoom3d_minmax_f32(const float* src, int sx, int sy, int sz, const fsg_tap* tx, const fsg_tap* ty,
                          const fsg_tap* tz, int dx, int dy, int dz, int32_t* mm, void* stream);
/* K9 pass B (+K10): mode 0: dst = y / max            (synthseg.py:112, what FetalSynthGen.sample returns)
 *                   mode 1: t = y / max; dst = (t - mn/max) / (1 - mn/max)   (+ data/datasets.py:311) */
int fsg_zoom3d_normalise_f32(const float* src, int sx, int sy, int sz, const fsg_tap* tx, const fsg_tap* ty,
                             const fsg_tap* tz, float* dst, int dx, int dy, int dz, const int32_t* mm,
                             int mode, void* stream);

/* Sharded form of the K9 pair (what fsg_sample_run uses): `slots` = nslots (2..64) slots of FSG_MM_SLOT_STRIDE int32 each,
 * slot s = {min key, max key, unused...}, every slot initialised by the caller to {key(+inf), key(-inf)} (the values
 * fsg_minmax_init writes).  The min/max pass updates slot (workgroup index % nslots); the normalise pass reduces the
 * slots itself.  Same results as the unsharded pair; the keys no longer sit on one contended address. */
#define FSG_MM_SLOT_STRIDE 16
int fsg_zoom3d_minmax_sharded_f32(const float* src, int sx, int sy, int sz, const fsg_tap* tx, const fsg_tap* ty,
                                  const fsg_tap* tz, int dx, int dy, int dz, int32_t* slots, int nslots, void* stream);
int fsg_zoom3d_normalise_sharded_f32(const float* src, int sx, int sy, int sz, const fsg_tap* tx, const fsg_tap* ty,
                                     const fsg_tap* tz, float* dst, int dx, int dy, int dz, const int32_t* slots, int nslots,
                                     int mode, void* stream);

/* ---- K2/K3: deformation coordinates (affine_nonrigid.py:64-84, :299-366) ----------------------- */
/* Reset six int32 keys to (+inf,+inf,+inf,-inf,-inf,-inf) / two keys to (+inf,-inf). */
int fsg_minmax_init(int32_t* mm, int npairs_min, int npairs_max, void* stream);
/* Optional accelerator for fsg_coords_minmax_f32 / fsg_warp_*: x/y-interpolate the coarse displacement grid
 * (and the coarse bias grid of `epi_host`, may be NULL) once per (x,y) column into `rows`
 * (shape[0]*shape[1]*row_stride floats, caller-owned workspace); then set d->rows / d->row_stride.
 * Results are bit-identical with or without it. */
int fsg_deform_rows_f32(const fsg_deform* d_host, const struct fsg_epilogue* epi_host, float* rows, int row_stride,
                        void* stream);
/* min / max over the grid of the clamped coordinates, before margin subtraction; mm6 = {min x,y,z,
 * max x,y,z} as ordered int32 keys.  Reads only the coarse field. */
int fsg_coords_minmax_f32(const fsg_deform* d_host, int32_t* mm6, void* stream);
/* What the warp actually needs: keys in mm3[0..2] whose floor equals floor(min) of the clamped coordinate
 * per axis (caller initialises them with fsg_minmax_init(mm3, 3, 0)).  Evaluates the six faces of the grid
 * first; the full pass exits immediately once every axis has a voxel below 1 (coordinates are >= 0, so
 * floor(min) is then 0).  Usable wherever fsg_warp_* takes `mm6` (only entries 0..2 are read there).
 * Returns FSG_E_TOOBIG for coarse grids beyond the row kernels' capacity: use fsg_coords_minmax_f32. */
int fsg_coords_floormin_f32(const fsg_deform* d_host, int32_t* mm3, void* stream);
/* Materialise xx2, yy2, zz2 (after subtracting floor(min)) -- the tensors
 * SpatialDeformation.generate_deformation_and_flip returns.  mm6 from fsg_coords_minmax_f32. */
int fsg_coords_f32(const fsg_deform* d_host, const int32_t* mm6, float* xx, float* yy, float* zz, void* stream);

/* ---- K3+K4(+K5) fused warp (affine_nonrigid.py:164-193 + utils/generation.py:204-288) ---------- */
/* For every voxel of the grid: recompute its sampling position from the coarse field (no coordinate
 * volumes in HBM), then
 *   out_lin = trilinear(src_lin)  (strict >0 validity, x->y->z blend, 0 outside)  [+ optional epilogue]
 *   out_nn  = nearest(src_nn)     (round-half-even, index clamp)
 * Either pair may be NULL.  Epilogue on out_lin (synthseg.py:274 and :178-182), each optional:
 *   gamma > 0:      v = 300 * (v/300)^gamma
 *   bias != NULL:   v = v * exp(zoom(bias))  with bias (b0,b1,b2) and per-axis tables bx,by,bz. */
typedef struct fsg_epilogue {
  float gamma;           /* <= 0: skip */
  int32_t bias_dims[3];
  const float* bias;     /* DEVICE, NULL: skip */
  const fsg_tap* bx;
  const fsg_tap* by;
  const fsg_tap* bz;
} fsg_epilogue;
int fsg_warp_f32(const fsg_deform* d_host, const int32_t* mm6, const float* src_lin, float* out_lin,
                 const float* src_nn, float* out_nn, const fsg_epilogue* epi_host, void* stream);
/* Same with uint8 label volumes for the nearest leg (device-resident streaming path). */
int fsg_warp_f32_u8(const fsg_deform* d_host, const int32_t* mm6, const float* src_lin, float* out_lin,
                    const uint8_t* src_nn, uint8_t* out_nn, const fsg_epilogue* epi_host, void* stream);

/* Label volume read as uint8, deformed labels written as float32 (exact for 0..255): the reference keeps
 * segmentations as float32 tensors, the device-resident copy is uint8.  Served by the lean warp kernel (per-row
 * coarse values prepared, coarse grids <= 32 entries along z, shape[2] <= 512) only; returns FSG_E_ALIGN otherwise
 * and the caller uses fsg_warp_f32 / fsg_warp_f32_u8. */
int fsg_warp_f32_u8_to_f32(const fsg_deform* d_host, const int32_t* mm6, const float* src_lin, float* out_lin,
                           const uint8_t* src_nn, float* out_nn, const fsg_epilogue* epi_host, void* stream);

/* The fused warp with a SECOND trilinear source in the same launch: out_img = trilinear(src_img) at the positions (and with the
 * in-kernel flip, the weights and the strict > 0 rule) of src_lin -> out_lin, float32, WITHOUT the epilogue, which stays on
 * out_lin alone.  The real image of a `load_image` sample beside its synthetic channel (affine_nonrigid.py:186-193 interpolates
 * output, segmentation and image on one set of coordinates): one launch instead of fsg_warp_* for (src_lin, src_nn) plus
 * fsg_warp_f32 for src_img alone, and bit for bit their three outputs.  img_voxels: the number of float32 elements behind
 * src_img AND out_img.  label_dtype_in / label_dtype_out: FSG_LABEL_F32 or FSG_LABEL_U8 of src_nn / out_nn (float32 -> float32,
 * uint8 -> uint8, uint8 -> float32); the label pair may be NULL.
 * FSG_E_BADARG, and nothing is launched: src_img without out_img or the reverse, src_img without src_lin, img_voxels different
 * from the grid's voxel count, out_img aliasing src_img / src_lin / out_lin, out_lin aliasing src_img, or any argument
 * fsg_warp_f32 refuses.
 * Served by the lean kernel alone (csrc/fsg_warp_lean.hip); FSG_E_ALIGN outside its domain or with it switched off
 * (fsg_set_tuning), and the caller issues the two launches. */
int fsg_warp_dual_f32(const fsg_deform* d_host, const int32_t* mm6, const float* src_lin, float* out_lin, const float* src_img,
                      float* out_img, size_t img_voxels, const void* src_nn, void* out_nn, int label_dtype_in,
                      int label_dtype_out, const fsg_epilogue* epi_host, void* stream);

/* Generic gather with explicit coordinate volumes (utils/generation.py:204-288 fast_3D_interp_torch).
 * mode 0 = linear (default_value outside), 1 = nearest.  src (sx,sy,sz); npts coordinates. */
int fsg_interp3d_f32(const float* src, int sx, int sy, int sz, const float* ii, const float* jj,
                     const float* kk, size_t npts, int mode, float default_value, float* dst, void* stream);

/* ---- K5 stand-alone (synthseg.py:250-275, :144-188) ------------------------------------------- */
int fsg_gamma_f32(const float* x, size_t n, float gamma, float* out, void* stream);
int fsg_bias_mul_f32(const float* x, int nx, int ny, int nz, const float* bias, int b0, int b1, int b2,
                     const fsg_tap* bx, const fsg_tap* by, const fsg_tap* bz, float* out, void* stream);

/* ---- K6: separable Gaussian blur, one axis pass (utils/generation.py:84-110) -------------------- */
/* dst = conv1d(src, taps) along `axis` with zero padding (no border renormalisation); ntaps odd.
 * taps: DEVICE pointer.  src != dst. */
int fsg_blur_axis_f32(const float* src, float* dst, int nx, int ny, int nz, int axis, const float* taps,
                      int ntaps, void* stream);
/* Tuned path: taps passed from HOST memory (copied into the kernel arguments, <= 129 taps).  Needs
 * 16-byte aligned volumes and a z extent that is a multiple of 4; returns FSG_E_ALIGN otherwise (the
 * caller then uses fsg_blur_axis_f32).  Same result contract as fsg_blur_axis_f32. */
int fsg_blur_axis_taps_host_f32(const float* src, float* dst, int nx, int ny, int nz, int axis,
                                const float* taps_host, int ntaps, void* stream);

/* y pass then z pass of the same blur in ONE launch (the intermediate volume stays in LDS): bit-identical to
 * fsg_blur_axis_taps_host_f32(axis 1) followed by (axis 2).  Serves identical taps on both axes (the isotropic blur of
 * RandResample), radius 1..8, 16-byte aligned volumes, nz % 4 == 0; FSG_E_ALIGN otherwise.  Algorithmic bytes: two passes (16 B/voxel) for 8 B/voxel of HBM traffic. */
int fsg_blur_yz_taps_host_f32(const float* src, float* dst, int nx, int ny, int nz, const float* taps_y_host, int ntaps_y,
                              const float* taps_z_host, int ntaps_z, void* stream);

/* ---- K8 stand-alone (synthseg.py:206-235) ------------------------------------------------------ */
int fsg_add_noise_f32(const float* x, size_t n, const float* noise, uint64_t seed, uint64_t stream_id,
                      float noise_std, float* out, void* stream);

/* ---- K9/K10 stand-alone reductions / scaling --------------------------------------------------- */
/* Empty inputs: in the entry points whose work is one flat range of `size_t n` elements, n == 0 is success with no launch
 * and outputs are not touched (one exception: fsg_gmm_sample_u8x4_mm with mm given still resets mm to its identities).
 * The n == 0 test comes first in every one of them, so pointers (and nlabels / ntab) are not looked at and may be null.
 * The calls that follow the rule are the K1/K5/K8/K9/K10 element-wise calls of this header
 * (fsg_gmm_sample_*, fsg_randn_f32, fsg_label_stats_*, fsg_gamma_f32, fsg_add_noise_f32, fsg_reduce_minmax_f32,
 * fsg_scale_f32, fsg_cast_f32_to_f16) and, of the artifact helpers, fsg_blend_f32, fsg_slice_noise_f32,
 * fsg_nonzero_count_* / fsg_nonzero_select_*, fsg_compact_f32, fsg_ewise_f32, fsg_boundary_mask_f32,
 * fsg_bernoulli_keep_f32 and fsg_scatter_const_f32.  Not covered, FSG_E_BADARG as before: every int dimension or count
 * (D, H, W, k, nreq, nvoid, ...); the slice size `hw` of fsg_slice_sums_f32 (the sum of an empty slice would have to be
 * written, which is a launch); fsg_copy_bytes (nbytes == 0); and the entry points that take n next to a plan or a table
 * it must agree with -- fsg_sample_head_f32, fsg_sample_head_codes_f32, fsg_equalize_f32, fsg_seed_codes_build,
 * fsg_seed_meta_pack -- where an empty volume can only be a caller's mistake.
 * NaN: fminf / fmaxf ignore it, so mm is the min / max of the non-NaN elements; an all-NaN (or empty) input leaves the
 * identities of fsg_minmax_init (+inf, -inf).  torch.min / max would return NaN; the generator never produces one here. */
int fsg_reduce_minmax_f32(const float* x, size_t n, int32_t* mm, void* stream); /* mm[0]=min key, mm[1]=max key */
/* mode 0: out = x / max;  mode 1: out = (x - min) / (max - min) (0*x if flat);  mode 2: (x-min)/(max-min)*255 */
int fsg_scale_f32(const float* x, size_t n, const int32_t* mm, int mode, float* out, void* stream);
/* dst[0..nbytes) = src[0..nbytes) by a kernel on `stream`; both 16-byte aligned, nbytes a multiple of 16.  `src` may be
 * pinned host memory: the per-sample parameter arena is uploaded this way so that the sample stays in one hardware queue. */
int fsg_copy_bytes(void* dst, const void* src, size_t nbytes, void* stream);
/* Decode ordered keys on the host side helper (pure function, no GPU). */
float fsg_key_to_float(int32_t key);

/* ---- SR-artifact slice-stack simulation ------------------------------------------------- */
/* Slice acquisition and its adjoint: the two operators of generator/artifacts/simulate_reco.py
 * (Scanner.scan :386-407 calls the forward, PSFreconstruction :38-54 the adjoint).  They replace the
 * reference's own CUDA extension, generator/artifacts/svort/slice_acquisition/slice_acq_cuda.cpp:22-160
 * (`forward`, `adjoint_forward`) and its kernels slice_acq_cuda_kernel.cu:17-171, :472-693.
 *   transforms (n,3,4) fp32 row-major [R|t], "translation first": p = R (pixel + t)
 *   vol (D,H,W) fp32, x fastest; psf (pd,ph,pw) fp32; slices (n,h,w) fp32
 *   vol_mask (D,H,W) / slices_mask (n,h,w): one byte per element (torch.bool), or NULL
 * mode selects which of the reference's two arithmetics is followed:
 *   FSG_SA_LINEAR      CUDA kernel, interp_psf=false: trilinear volume sample per PSF tap (:110-161, :607-666)
 *   FSG_SA_NEAREST_PSF CUDA kernel, interp_psf=true : nearest voxel (round half away from zero), PSF
 *                      re-interpolated at that voxel (:71-109, :572-605)
 *   FSG_SA_TORCH       the CPU fallback slice_acq.py:266-546 (nearest voxel by round-half-even, strict inside
 *                      test, raw PSF taps > 0, normalisation where weight > 1e-2, no per-pixel weight in the adjoint);
 *                      a 1x1x1 PSF without slices_weight takes the fallback's grid_sample route (slice_acq.py:381-384,
 *                      :445-480: trilinear, zero padding, slices_mask applied) in the forward
 * PSF limits: each extent <= 64, pd*ph*pw <= 4096 (it is staged in LDS), else FSG_E_TOOBIG. */
#define FSG_SA_LINEAR 0
#define FSG_SA_NEAREST_PSF 1
#define FSG_SA_TORCH 2
/* slices = A(vol) / weight where weight > 0 (CUDA modes; > 1e-2 in FSG_SA_TORCH), 0 elsewhere and outside
 * slices_mask; slices_weight (may be NULL) receives the weights.  Every element of both outputs is written. */
int fsg_slice_acq_forward_f32(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf, int pd,
                              int ph, int pw, const uint8_t* slices_mask, float* slices, float* slices_weight, int D, int H,
                              int W, int n, int h, int w, float res_slice, int mode, void* stream);
/* vol = A^T(slices), vol_weight = A^T(1) (may be NULL).  CUDA modes skip pixels whose PSF weight inside the volume is
 * < 0.5 and divide each contribution by that weight (:560, :600, :616).  Two entries, two accumulation rules:
 *   fsg_slice_acq_adjoint_f32      both outputs are zeroed by the call, then accumulated with fp32 atomics, as the
 *                                  reference does: the summation order, and with it the last bits of the result, differ
 *                                  from run to run and with fsg_slice_acq_set_tuning.  NOT deterministic.
 *   fsg_slice_acq_adjoint_det_f32  deterministic: the result is a pure function of the inputs (below).
 * slice_ids (DEVICE, n x int32, may be NULL): transform z of the launch applies to slices[slice_ids[z]] (and that
 * row of slices_mask) -- the reconstruction keeps a random subset of the slices (simulate_reco.py:768-769)
 * without copying them.
 * Equalisation is a separate launch (fsg_equalize_f32), as in the reference (:1062-1074). */
int fsg_slice_acq_adjoint_f32(const float* transforms, const float* psf, int pd, int ph, int pw, const float* slices,
                              const uint8_t* slices_mask, const int32_t* slice_ids, const uint8_t* vol_mask, float* vol,
                              float* vol_weight, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                              void* stream);
/* The deterministic adjoint (FSG_SA_LINEAR and FSG_SA_NEAREST_PSF; FSG_SA_TORCH is refused with FSG_E_BADARG).
 * The rule, with F = FSG_SA_DET_FRAC_BITS = 72 and L = FSG_SA_DET_LIMB_BITS = 40:
 *   1. every contribution is formed in fp32 as in the float entry's LDS kernel: c_w = pv' = pv * (1 / wsum) (times the
 *      trilinear corner weight in FSG_SA_LINEAR), c_v = fl32(c_w * s) for the pixel value s;
 *   2. it becomes an integer with ONE rounding: Q_v = rint_half_even(c_v * 2^F / value_scale), Q_w = rint_half_even(c_w * 2^F)
 *      (the scaling by a power of two is exact).  A contribution of 2^-(F-24) = 2^-48 and more is an exact multiple of
 *      2^-F: it enters exactly, smaller ones with an error of at most 2^-(F+1);
 *   3. Q is carried as two 64-bit limbs, Q = hi * 2^L + lo with hi = rint_half_even(c * 2^(F-L)), |lo| <= 2^(L-1); the limbs
 *      are added with 64-bit integer atomics, in LDS and in `ws`, each on its own.  Integer addition is associative, so
 *      the sums do not depend on the order;
 *   4. a last pass forms sum(hi) * 2^L + sum(lo) exactly and converts it with ONE rounding, integer -> float32 to nearest
 *      even, then multiplies by 2^-F * value_scale (2^-F for the weight), which is exact.  An accumulator nothing was
 *      added to gives +0.0f.
 *   The per-pixel weight wsum of the CUDA modes follows the same idea in one limb: each tap's PSF value is quantised to
 *   2^-32, the integers are summed, and the sum is converted once; the < 0.5 cut and 1 / wsum use that float.
 * vol and vol_weight are therefore bit-identical for the same inputs under any fsg_slice_acq_set_tuning setting, under
 * FSG_TUNE_SA_DIRECT, for any order of the slices, for slice_ids against gathered slices, on any stream and in any run.
 * Why two limbs and not one int64 at 2^-32: equalisation divides value by weight wherever the weight is > 0, and voxels that
 * only the fringe of a PSF (or a trilinear corner weight near 0) reaches have weights of a few times 2^-32 and less; their
 * quotient would be noise.  At 2^-72 value and weight are the exact sums of the fp32 contributions for every contribution
 * of 2^-48 and more, rounded once: closer to the real sum than any fp32 summation order.
 *   value_scale  a power of two in [2^-20, 2^20], else FSG_E_BADARG; 1 for slices scaled to about [0, 1].  It is given by
 *                the caller, not derived from the data: a data-derived scale would tie the bits to which slices are passed.
 *   range        per voxel |sum of weights| and |sum of values / value_scale| must stay below 2^(63-(F-L)) = 2^31 and the
 *                number of contributions below 2^(63-L) = 2^23; the generator's geometry stays below 2^21 and 2^22
 *                (DESIGN section 17).  Beyond the range the sums wrap (no fault).
 *   ws           DEVICE, 8-byte aligned (else FSG_E_ALIGN), ws_bytes >= fsg_slice_acq_adjoint_det_ws_bytes(D, H, W,
 *                vol_weight != NULL) = 16 * D*H*W bytes, twice that with weights; zeroed by the call on `stream`.
 * Every refusal leaves vol, vol_weight and ws untouched; otherwise every element of vol (and vol_weight) is written.
 * Non-finite slice values give unspecified values in the voxels they reach and never a fault: no address depends on them.
 * Equalisation stays the separate fsg_equalize_f32 launch on the converted floats. */
#define FSG_SA_DET_FRAC_BITS 72
#define FSG_SA_DET_LIMB_BITS 40
size_t fsg_slice_acq_adjoint_det_ws_bytes(int D, int H, int W, int want_weight);
int fsg_slice_acq_adjoint_det_f32(const float* transforms, const float* psf, int pd, int ph, int pw, const float* slices,
                                  const uint8_t* slices_mask, const int32_t* slice_ids, const uint8_t* vol_mask, float* vol,
                                  float* vol_weight, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                                  void* ws, size_t ws_bytes, float value_scale, void* stream);
/* Shape of the LDS pre-summation of the FSG_SA_NEAREST_PSF adjoint: accumulator cells (value + weight, 8 B each,
 * 256..18432), PSF planes per chunk, and the footprint (pixel pitch * 15 + PSF width, voxels) up to which 16x16-pixel
 * tiles are used instead of 8x8.  z_chunk 0 (default) derives the planes per chunk, and a larger capacity when one
 * plane does not fit, from the pixel pitch and the PSF size.  Defaults 3072 / 0 / 20.  Results do not depend on it beyond fp32 summation order.
 * The deterministic entry reads the same three values with cells of 32 B and at most 4096 of them; its results do not
 * depend on them at all. */
int fsg_slice_acq_set_tuning(int cap_cells, int z_chunk, int t16_extent);
/* vol[i] /= vol_weight[i] where vol_weight[i] > threshold (0 for the CUDA kernel :681-691, 1e-2 for the
 * fallback slice_acq.py:542-543); then vol[i] *= vol_mask[i] if vol_mask (fallback :544-545).  Either of
 * vol_weight / vol_mask may be NULL, not both. */
int fsg_equalize_f32(float* vol, const float* vol_weight, const uint8_t* vol_mask, float threshold, size_t n, void* stream);
/* Backward of fsg_slice_acq_forward_f32 (fsg_slice_acq_bwd.hip; reference SliceAcqFunction.backward,
 * slice_acq_cuda_kernel.cu:173-470): grad_vol (D,H,W) and grad_transforms (n,12) from grad_slices (n,h,w).  Either output
 * may be NULL (not both: FSG_E_BADARG).  FSG_SA_LINEAR and FSG_SA_NEAREST_PSF; FSG_SA_TORCH is refused with FSG_E_BADARG
 * (the fallback has no backward of its own).  PSF limits as the forward.  The rule is the reference's, quirks included:
 *   - a pixel outside slices_mask, or with grad_slices == 0, contributes nothing;
 *   - pass 1: weight = sum over the taps inside the volume (0 <= p < size - 1 per axis) of the raw PSF value (LINEAR) or of
 *     the PSF re-interpolated at the rounded voxel, taps outside the PSF grid skipped (NEAREST_PSF).  vol_mask is NOT
 *     consulted here, although the forward's own weight leaves masked voxels out; weight == 0 ends the pixel (the forward
 *     tests weight > 0), otherwise gs = grad_slices / weight;
 *   - pass 2, grad_vol: LINEAR adds gs * psf * corner weight to the up-to-8 unmasked corners, NEAREST_PSF gs * psf' to the
 *     rounded voxel if it is unmasked;
 *   - pass 2, grad_transforms: d = gs * (derivative of the trilinear weights with respect to the sampling position) summed
 *     over the same unmasked terms, the weight held constant.  LINEAR: d is in volume axes, g_R[a][b] += d[a] * l[b] with
 *     the lever l = pixel + translation + tap offset in slice axes, g_t += R^T d.  NEAREST_PSF: d is in PSF axes,
 *     g_R[a][b] += l[a] * d[b] with l = rounded voxel - volume centre, g_t -= d.
 *   Arithmetic is fp32 in the reference's operation order except that the NEAREST_PSF lever products are formed in fp32
 *   (the reference promotes them to double through a literal).
 * Accumulation:
 *   grad_vol         zeroed by the call on `stream`, then fp32 vector atomics, as the reference and fsg_slice_acq_adjoint_f32:
 *                    the order of the additions, and with it the last bits, change from run to run.  NOT deterministic
 *                    (bit-identical only where a voxel receives at most one contribution).  fsg_slice_acq_backward_det_f32
 *                    below sums the same contributions in fixed point and is deterministic.
 *   grad_transforms  DETERMINISTIC, no atomics: 12 sums per thread in registers, a fixed shuffle tree per wave, the waves of a
 *                    workgroup added in order through LDS, one 12-float partial per workgroup stored at ws[slice][tile], and a
 *                    second launch that adds a slice's tiles in index order.  The same bits on any stream, in any run, and
 *                    with grad_vol requested or not.
 *   ws               DEVICE; read and written only when grad_transforms is requested, and then it must be 8-byte aligned
 *                    (else FSG_E_ALIGN) with ws_bytes >= fsg_slice_acq_backward_ws_bytes(n, h, w) = 48 bytes per 16x16 pixel
 *                    tile of every slice (else FSG_E_BADARG).  It needs no initialisation.
 * Every refusal leaves grad_vol, grad_transforms and ws untouched; otherwise every element of each requested output is written.
 * No allocation and no host synchronisation inside.  Every in-volume and in-PSF test accepts (`!(p >= 0 && p < size - 1)`
 * skips), so a NaN or Inf in transforms or res_slice skips the tap: no address depends on a value that failed a range test.
 * Non-finite vol, psf or grad_slices values give unspecified values where they reach and never a fault. */
size_t fsg_slice_acq_backward_ws_bytes(int n, int h, int w);
int fsg_slice_acq_backward_f32(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf, int pd,
                               int ph, int pw, const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                               float* grad_transforms, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                               void* ws, size_t ws_bytes, void* stream);
/* The same backward with a DETERMINISTIC grad_vol (FSG_SA_LINEAR and FSG_SA_NEAREST_PSF; FSG_SA_TORCH is refused with
 * FSG_E_BADARG).  Only the accumulation of grad_vol differs from fsg_slice_acq_backward_f32.  The rule, with
 * F = FSG_SA_DET_FRAC_BITS = 72 and L = FSG_SA_DET_LIMB_BITS = 40, as for fsg_slice_acq_adjoint_det_f32:
 *   1. a contribution is the float32 value fsg_slice_acq_backward_f32 hands to its atomic, formed by the same fp32 operations
 *      in the same order (no FMA contraction): FSG_SA_NEAREST_PSF c = fl32(psf' * gs), psf' the eight-term trilinear sum of
 *      the PSF at the rounded voxel; FSG_SA_LINEAR c = fl32(fl32(fl32(fx * fy) * fz) * fl32(psf * gs)) per unmasked corner.
 *      Pass 1, weight, the weight != 0 test, gs = grad_slices / weight, the masks and the accepting range tests are those
 *      above, quirks included;
 *   2. it is quantised ONCE, Q = rint_half_even(c * 2^F / grad_scale) (the scaling by a power of two is exact), carried as
 *      two 64-bit limbs Q = hi * 2^L + lo, hi = rint_half_even(c * 2^(F-L) / grad_scale), |lo| <= 2^(L-1), and each limb is
 *      added on its own with a 64-bit integer atomic into det_ws, 2 limbs per voxel (a limb that is zero is not sent).
 *      Integer addition is associative, so the sums do not depend on the order.  A contribution of 2^-48 * grad_scale and
 *      more enters exactly, a smaller one with an error of at most 2^-(F+1) * grad_scale;
 *   3. a finalising pass forms sum(hi) * 2^L + sum(lo) exactly, rounds it ONCE to float32 (nearest even) and multiplies by
 *      2^-F * grad_scale, which is exact.  It writes every voxel; an accumulator nothing was added to gives +0.0f;
 *   4. grad_scale is a power of two in [2^-20, 2^20] (else FSG_E_BADARG), 1 for gradients of about unit size.  It is given
 *      by the caller and never derived from the data: a data-derived scale would tie the bits of one voxel to every other
 *      slice that is passed.  Range per voxel: |sum of contributions / grad_scale| < 2^(63-(F-L)) = 2^31 and fewer than
 *      2^(63-L) = 2^23 contributions; beyond it the sums wrap (no fault);
 *   5. grad_transforms is untouched: it has the bits of fsg_slice_acq_backward_f32, whether or not grad_vol is requested.
 * grad_vol is therefore bit-identical for the same inputs in any run, on any stream, for any order of the slices (transforms,
 * grad_slices and slices_mask permuted together) and with or without grad_transforms.
 *   ws      as fsg_slice_acq_backward_f32: needed only when grad_transforms is requested.
 *   det_ws  DEVICE; needed only when grad_vol is requested (else it may be NULL), and then 8-byte aligned (else FSG_E_ALIGN)
 *           with det_ws_bytes >= fsg_slice_acq_backward_det_ws_bytes(D, H, W) = 16 bytes per voxel (else FSG_E_BADARG);
 *           zeroed by the call on `stream`.
 * Every refusal leaves grad_vol, grad_transforms, ws and det_ws untouched; otherwise every element of each requested output
 * is written.  No allocation and no host synchronisation inside.  Non-finite grad_slices, vol or psf values give unspecified
 * values where they reach and never a fault: no address depends on a value that did not pass a range test. */
size_t fsg_slice_acq_backward_det_ws_bytes(int D, int H, int W);
int fsg_slice_acq_backward_det_f32(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf, int pd,
                                   int ph, int pw, const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                                   float* grad_transforms, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                                   void* ws, size_t ws_bytes, void* det_ws, size_t det_ws_bytes, float grad_scale,
                                   void* stream);
/* Backward of fsg_slice_acq_adjoint_f32 + fsg_equalize_f32 (fsg_slice_acq_adjoint_bwd.hip; reference
 * SliceAcqAdjointFunction.backward, slice_acq_cuda_kernel.cu:695-950, host side :1079-1132): grad_slices (n,h,w) and
 * grad_transforms (n,12) from grad_vol (D,H,W).  Either output may be NULL (not both: FSG_E_BADARG).  FSG_SA_LINEAR and
 * FSG_SA_NEAREST_PSF; FSG_SA_TORCH is refused with FSG_E_BADARG.  PSF limits as the forward.  `equalize` != 0 is the backward
 * of the equalised adjoint and needs vol_weight (the adjoint's weight output) and vol (its EQUALISED output), else
 * FSG_E_BADARG; without it both are ignored and may be NULL.  The rule is the reference's, quirks included:
 *   - equalisation of the gradient (:672-693, is_grad = true): g'[i] = grad_vol[i] / (w < 1e-3 ? 1e-3 : w) where
 *     w = vol_weight[i] > 0, g'[i] = grad_vol[i] elsewhere; the comparison with and the division by the literal 1e-3 are done
 *     in double, as the reference's promotion does, the division by w in fp32.  The reference overwrites the incoming gradient;
 *     here one streaming pre-pass writes g' into ws and grad_vol is NEVER written.  Without equalize g' = grad_vol, no copy;
 *   - a pixel outside slices_mask contributes nothing.  Otherwise ONE pass over the non-zero PSF taps whose position is inside
 *     the volume (0 <= p < size - 1 per axis); geometry as fsg_slice_acq_adjoint_f32;
 *   - LINEAR: val_ = sum over the unmasked corners of corner weight * g'[corner]; val += psf * val_; weight += psf -- the tap
 *     counts whatever vol_mask says.  Transforms: per unmasked corner s = (equalize ? slices[p] - vol[corner] : slices[p]) *
 *     g'[corner]; d = psf * sum of s * (derivative of the corner weight with respect to the position), in volume axes;
 *     g_R[a][b] += d[a] * l[b] with the lever l = pixel + translation + tap offset in slice axes, g_t += R^T d;
 *   - NEAREST_PSF: the voxel is the rounded position (half away from zero).  A voxel outside vol_mask skips the tap BEFORE it
 *     is added to weight; then the PSF is re-interpolated at the rounded voxel, taps whose PSF coordinate leaves
 *     [0, psf_size - 1) skipped; val += psf' * g'[voxel]; weight += psf'.  Transforms: d = (derivative of psf' with respect
 *     to the PSF coordinate, from its 8 PSF neighbours) * s, s = (equalize ? slices[p] - vol[voxel] : slices[p]) * g'[voxel],
 *     in PSF axes; g_R[a][b] += l[a] * d[b] with l = rounded voxel - volume centre, g_t -= d;
 *   - end of pixel: weight > 0 gives grad_slices[p] = val / weight and the pixel's 12 sums divided by weight; otherwise
 *     the pixel gives nothing.
 *   Quirks kept: (1) the adjoint forward drops pixels with weight < 0.5, this backward tests weight > 0; (2) in NEAREST_PSF
 *   with a vol_mask the forward's per-pixel weight counts masked voxels and this one does not; (3) the per-pixel weight is
 *   treated as a constant in grad_transforms; (4) the 1e-3 floor.  So this is the derivative of the adjoint only where every
 *   kept pixel has weight >= 0.5 and, in NEAREST_PSF, there is no vol_mask.
 *   Arithmetic is fp32 in the reference's operation order except that the NEAREST_PSF lever products are formed in fp32
 *   (the reference promotes them to double through a literal), as fsg_slice_acq_backward_f32.
 * DETERMINISTIC, both outputs: the kernel only gathers.  grad_slices is one plain store per pixel; grad_transforms takes the
 * reduction of fsg_slice_acq_backward_f32 (12 register sums, a fixed shuffle tree per wave, waves in order through LDS, one
 * 12-float partial per workgroup in ws, a second launch adding a slice's tiles in index order).  No atomics.  The same bits on
 * any stream, in any run, and for one output whether or not the other is requested.
 *   ws   DEVICE; fsg_slice_acq_adjoint_backward_ws_bytes(D, H, W, n, h, w, equalize, want_transforms) = 48 bytes per 16x16
 *        pixel tile of every slice if grad_transforms is requested, plus 4 * D*H*W if equalize.  If that is 0, ws is not
 *        touched and may be NULL; otherwise it must be 8-byte aligned (else FSG_E_ALIGN) and large enough (else FSG_E_BADARG).
 *        It needs no initialisation.
 * Every refusal leaves grad_slices, grad_transforms and ws untouched; otherwise every element of each requested output is
 * written: 0 outside slices_mask and where weight <= 0.  No allocation and no host synchronisation inside.  Every in-volume and
 * in-PSF test accepts (`!(p >= 0 && p < size - 1)` skips), so a NaN or Inf in transforms or res_slice skips the tap and the
 * pixel gives zeros: no address depends on a value that failed a range test.  Non-finite grad_vol, vol, vol_weight, psf or
 * slices values give unspecified values where they reach and never a fault. */
size_t fsg_slice_acq_adjoint_backward_ws_bytes(int D, int H, int W, int n, int h, int w, int equalize, int want_transforms);
int fsg_slice_acq_adjoint_backward_f32(const float* transforms, const float* grad_vol, const float* vol_weight /*equalize*/,
                                       const float* vol /*equalize: the equalised output of the forward*/,
                                       const uint8_t* vol_mask, const float* psf, int pd, int ph, int pw, const float* slices,
                                       const uint8_t* slices_mask, float* grad_slices /*may be NULL*/,
                                       float* grad_transforms /*may be NULL; not both*/, int D, int H, int W, int n, int h,
                                       int w, float res_slice, int mode, int equalize, void* ws, size_t ws_bytes, void* stream);

/* ---- pose conversions (fsg_transform_convert.hip; reference svort/transform/transform_convert_cuda.cpp and
 * transform_convert_cuda_kernel.cu:14-440) ------------------------------------------------------
 * axisangle rows are [rotation vector (3) | translation (3)], mat rows the 12 entries of [R | t] in row-major order; both
 * fp32, C-contiguous, n rows.  One thread per row, 256 per workgroup; fp32 in the reference's operation order.
 *   fsg_axisangle2mat_f32           Rodrigues' formula for |rotation vector|^2 > 1e-6, else the first-order matrix I + [a]x.
 *   fsg_axisangle2mat_backward_f32  its derivative in both branches (small branch: the antisymmetric differences of grad_mat).
 *   fsg_mat2axisangle_f32           the quaternion by one of four formulas (chosen by r22 < 1e-6, r00 > r11, r00 < -r11), its
 *                                   sign flipped where w < 0, then the rotation vector (x,y,z) * fac with fac = theta / sin for
 *                                   x^2 + y^2 + z^2 > 1e-6, else 2 / w.
 *   fsg_mat2axisangle_backward_f32  the chain rule through that, all 12 entries of a row free.  QUIRK kept from the reference:
 *                                   for x^2 + y^2 + z^2 <= 1e-6 it differentiates fac as in the other branch with sin floored
 *                                   by 1e-6 (in double), which is NOT the derivative of 2 / w; elsewhere it is the derivative.
 * The comparisons with 1e-6 are float-with-double as in the reference.  No float lies between float(1e-6) and 1e-6, so they
 * agree with the float32 comparisons against float(1e-6) for every float32 value, except `r22 < 1e-6` at r22 == float(1e-6).
 * n == 0: returns 0 without a launch.  n < 0 or a null pointer with n > 0: FSG_E_BADARG.  12 * n > 2^31 - 1: FSG_E_TOOBIG.
 * An output that shares a byte with an input: FSG_E_BADARG (the kernels take their pointers __restrict__).  Every refusal
 * comes before any launch and leaves the output untouched; otherwise EVERY element of the output is written (the translation
 * column or elements copied bit for bit), so it needs no initialisation.  No address depends on a value: a NaN or Inf in a row
 * gives NaN or Inf in that row's output and nothing else (but a NaN pose given to fsg_axisangle2mat_backward_f32 compares
 * false, takes the small branch, which reads grad_mat alone, and leaves a finite row, as in the reference).  Deterministic: a
 * row's output is a function of that row alone. */
int fsg_axisangle2mat_f32(const float* axisangle /*(n,6)*/, float* mat /*(n,12)*/, int n, void* stream);
int fsg_axisangle2mat_backward_f32(const float* grad_mat /*(n,12)*/, const float* axisangle /*(n,6)*/,
                                   float* grad_axisangle /*(n,6)*/, int n, void* stream);
int fsg_mat2axisangle_f32(const float* mat /*(n,12)*/, float* axisangle /*(n,6)*/, int n, void* stream);
int fsg_mat2axisangle_backward_f32(const float* mat /*(n,12)*/, const float* grad_axisangle /*(n,6)*/,
                                   float* grad_mat /*(n,12)*/, int n, void* stream);

/* ---- conjugate gradients between two applications of the slice-acquisition operators (fsg_cg.hip) ----
 * The vector half of K = n_iter iterations of CG on M x = rhs, M p = V (A^T P W A (V p) + mu p), rhs = V (b + mu z):
 * the caller applies A and A^T (fsg_slice_acq_forward_f32, fsg_ewise_f32 op 3, fsg_slice_acq_adjoint[_det]_f32) and hands the
 * result `t` to these entries.  All vectors are fp32 with n elements; `mask` is V, one byte per voxel (non-zero keeps), or NULL.
 * One solve is the launch sequence
 *     init;  for k = 1..K:  t = A^T P W A p;  q(k);  step(k);  dir(k)
 * and it is the same sequence whatever the data: nothing returns early, nothing is read back.
 *   init     r = V(b + mu z) - V(t0 + mu x0) (second term only with x0; t0 = A^T P W A x0), p = r, x = V x0 or 0.  z may be NULL.
 *   q(k)     q = V(t + mu p), written over t.
 *   step(k)  alpha[k] = (float)(rr[k-1] / pq[k]);  x = x + alpha p;  r = r - alpha q (r is not stored when k == K).
 *   dir(k)   beta[k] = (float)(rr[k] / rr[k-1]);  p = r + beta p (p is not touched when k == K).
 * Element-wise arithmetic is fp32, one rounding per operation (no contraction); V is a selection (a masked element is +0).
 * Scalars: ws holds, 8-byte aligned and in this order, with s = K + 1 and B = clamp(ceil(n / 1024), 1, 1024):
 *     double rr[s], double pq[s], double partial_rr[B], double partial_pq[B], float alpha[s], float beta[s], int32 frozen[s]
 * = fsg_cg_ws_bytes(n, K) bytes (rounded up to 8; 0 for K outside 1..FSG_SOLVER_MAX_ITER).  Slot k belongs to iteration k (slot 0 of pq, alpha,
 * beta is 0).  It needs no initialisation: q(1) writes rr[0], frozen[0] and the zero slots, step(k) writes pq[k] and alpha[k], dir(k) writes
 * rr[k], beta[k] and frozen[k], each from workgroup 0; a launch reads only slots and partials that an EARLIER launch wrote.
 * Dot products <r,r> and <p,q>: every launch has B workgroups of 256 threads.  Elements are dealt in groups of four: group
 * g = e / 4 belongs to thread g mod (256 B) (thread id = 256 workgroup + thread), whether it is loaded as one 16-byte word or
 * as scalars.  A thread adds (double)a[e] * (double)b[e] (exact) over its elements in increasing e, from +0.0; the 64 lanes of a
 * wave fold by the butterfly v[i] = v[i] + v[i ^ o] for o = 32, 16, 8, 4, 2, 1; thread 0 adds the 4 waves as ((w0 + w1) + w2) + w3
 * and stores one double per workgroup.  The NEXT launch that needs the sum adds the B partials in index order from +0.0, in
 * every workgroup alike.  No atomics, no second launch, no grid barrier: the sum is a function of the two arrays alone.
 * Freeze instead of early return: frozen[0] = rr[0] <= tol, frozen[k] = frozen[k-1] || !(pq[k] > 0) || rr[k] <= tol.
 *   - frozen[k-1]: q(k), step(k), dir(k) write no vector; pq[k] = 0, alpha[k] = beta[k] = 0, rr[k] = rr[k-1].
 *   - !(pq[k] > 0) (a NaN, or a direction M maps to 0): step(k) and dir(k) write no vector; x is what it was after k - 1 steps.
 *   - rr[k] <= tol: step(k) has updated x and r; dir(k) leaves p.
 *   x therefore holds exactly what a loop with `return` at those points returns, and a NaN never reaches another voxel.
 * FSG_CG_RELU in `flags` of step(K), the LAST iteration and only there: x = max(x, 0) once, in the same pass as the update, or
 * as the only thing the launch does when the solve is frozen by then.  For k < K the flag is ignored.
 * Loads and stores are 16 bytes per lane when every float pointer of the call is 16-byte aligned and mask is 4-byte aligned;
 * otherwise scalars, same values and same sums.
 * Refusals, all before any launch and with nothing written: K outside 1..FSG_SOLVER_MAX_ITER or k outside 1..K (FSG_E_BADARG); n == 0 is
 * success without a launch; a null vector or ws with n > 0, x0 without t0, ws_bytes < fsg_cg_ws_bytes(n, K), an unknown flag
 * (FSG_E_BADARG); ws not 8-byte aligned (FSG_E_ALIGN); an output that shares a byte with an input, another output or ws
 * (FSG_E_BADARG; q over t is the one in-place pair). */
#define FSG_CG_RELU 1
#define FSG_SOLVER_MAX_ITER 4096 /* the most iterations of one solve: K of fsg_cg_* and fsg_svr_update_f32, T of fsg_robust_* */
size_t fsg_cg_ws_bytes(size_t n, int n_iter);
int fsg_cg_init_f32(const float* b, const float* z, const float* t0, const float* x0, const uint8_t* mask, float mu, size_t n,
                    int n_iter, float* r, float* p, float* x, void* ws, size_t ws_bytes, void* stream);
int fsg_cg_q_f32(const float* p, float* t, const uint8_t* mask, float mu, double tol, size_t n, int k, int n_iter, void* ws,
                 size_t ws_bytes, void* stream);
int fsg_cg_step_f32(const float* p, const float* q, float* x, float* r, size_t n, int k, int n_iter, int flags, void* ws,
                    size_t ws_bytes, void* stream);
int fsg_cg_dir_f32(const float* r, float* p, double tol, size_t n, int k, int n_iter, void* ws, size_t ws_bytes, void* stream);

/* ---- first-order regulariser of the solve above (fsg_tk1.hip) ---------------------------------------
 *     out = t + lam * L p        over (D,H,W) fp32 volumes, W fastest
 * L = D^T C D is the weighted graph Laplacian of the 6-neighbour grid.  An edge (i, j) takes part iff both ends are inside the
 * volume and, with `mask` (V, one byte per voxel, non-zero keeps; NULL = all), both ends are in V: the free boundary follows the
 * mask.  Edge weight c = 1 without `guide`; with `guide` g and delta > 0 it is Huber's, a = |fl(g_i - g_j)|,
 * c = (a <= delta) ? 1 : fl(delta / a).  a has the same bits from either end of an edge, so L is symmetric entry for entry.
 * Per voxel i, fp32 with one rounding per operation (no contraction; the division is correctly rounded):
 *     acc = +0;  for the neighbours j in the order x-, x+, y-, y+, z-, z+ (x along W, z along D) that take part (the others
 *     are skipped, they do not contribute a zero):  d = fl(p_i - p_j);  with a guide d = fl(c * d);  acc = fl(acc + d);
 *     out_i = fl(t_i + fl(lam * acc)).
 * A voxel outside V gets out_i = t_i (fsg_cg_q_f32 / fsg_cg_init_f32 apply V afterwards).  A gather in a fixed order: the same
 * bits in any run and on any stream.  Four consecutive voxels per thread; 16-byte loads and stores when every float pointer of
 * the call is 16-byte aligned and mask 4-byte aligned (the neighbour rows too when W % 4 == 0), scalars otherwise, same values.
 * `out` may be `t` itself (in place).  Refusals, before any launch and with nothing written: a null p, t or out; D, H or W < 1;
 * lam not finite or < 0; with a guide, delta not finite or <= 0 (without one delta is ignored); out sharing a byte with p,
 * guide or mask, or overlapping t other than out == t (FSG_E_BADARG); D * H * W > 2^31 - 1 (FSG_E_TOOBIG). */
int fsg_tk1_apply_f32(const float* p, const float* t, const uint8_t* mask, const float* guide, float delta, float lam, int D,
                      int H, int W, float* out, void* stream);

/* ---- per-slice Levenberg-Marquardt slice-to-volume registration (fsg_svr.hip) ----------------------
 * One solve is the launch sequence, for k = 0..K (K = n_iter), all on one stream:
 *     transforms = axisangle2mat(theta_trial);  jac = d transforms / d theta at theta_trial;  normal;  update(k)
 * and it is the same sequence whatever the data: nothing returns early, nothing is read back.
 *
 * fsg_svr_normal_f32: the per-slice normal equations of the residual e = s - y, s the slice fsg_slice_acq_forward_f32 simulates
 * in FSG_SA_LINEAR without a vol_mask (any other `mode`: FSG_E_BADARG; there is no vol_mask parameter because the forward and
 * its backward treat one differently, so a Jacobian under a mask would not be the derivative of the residual).
 *   transforms (n,12), jac (n,12,6): row k of a slice = the derivative of transform entry k with respect to the 6 pose
 *   parameters; vol (D,H,W); psf (pd,ph,pw), limits as the forward; slices (n,h,w) = y; slices_mask (n,h,w) bytes or NULL;
 *   slices_weight (n,h,w) non-negative or NULL (w = 1); min_weight >= 0 (negative or NaN: FSG_E_BADARG).
 *   stats (n,32) DOUBLE (a row is FSG_SVR_SLOTS wide), 8-byte aligned: [0..20] H = sum w J J^T, upper triangle row-major (00 01 .. 05 11 12 .. 55);
 *   [21..26] g = sum w e J; [27] sum w e^2; [28] sum w; [29] m, the number of pixels that took part; [30], [31] = 0.
 * Per pixel inside slices_mask:
 *   pass 1  weight = the raw PSF sum over the non-zero taps with 0 <= p < size - 1 on every axis, exactly as
 *           fsg_slice_acq_backward_f32 in LINEAR.  The pixel takes part iff weight > 0 && weight >= min_weight.
 *   pass 2  over the same taps: tri = the eight-term trilinear sample of vol (corner order of the family, added to 0),
 *           val += psf * tri; and the twelve sums J12[k] that fsg_slice_acq_backward_f32 forms for grad_slices = 1, i.e.
 *           gs = 1 / weight, pg = psf * gs, per corner the derivative terms of pg * vol[corner], then the LINEAR lever arms:
 *           the same fp32 operations in the same order, the weight held constant.
 *   then    s = val / weight; e = s - y; J6[a] = sum_k jac[k][a] * J12[k], k increasing, from +0; we = w * e; the 30 fp32
 *           terms fl(fl(w * J6[a]) * J6[b]) (a <= b), we * J6[a], we * e, w, 1.  A pixel that takes no part carries 30 zeros.
 * Reduction, no atomics: the 64 lanes of a wave fold each term by v[i] += v[i + o], o = 32..1 (shuffle-down; lane 0 holds the
 * sum); the four waves of the 16x16 workgroup are added in wave order; the workgroup stores one 32-float partial (128 bytes)
 * at ws[slice][tile], tile = tile_y * tiles_x + tile_x; a second launch adds a slice's partials in DOUBLE in tile-index order
 * from +0.0 and writes all 32 slots.  stats of a slice is a pure function of that slice's inputs: the same bits in any run, on
 * any stream, for any order or number of the other slices.
 *   ws  DEVICE, 8-byte aligned (else FSG_E_ALIGN), ws_bytes >= fsg_svr_ws_bytes(n, h, w) = 128 bytes per 16x16 tile of every
 *       slice (else FSG_E_BADARG).  It needs no initialisation.
 * Every refusal (null pointer, bad size, PSF limits, mode, min_weight, alignment, short workspace) comes before the first
 * write and leaves stats and ws untouched.  No allocation and no host synchronisation inside.  Range tests accept, so a NaN or
 * Inf in transforms or res_slice skips the tap; non-finite vol, psf, jac, slices or weights give unspecified sums and never
 * an address.
 *
 * fsg_svr_update_f32: the damped step and the accept / reject decision for slot k of 0..K, one thread per slice, double
 * arithmetic with + - * / only and no contraction.  `state` is a DEVICE block of fsg_svr_state_bytes(n, K) bytes (0 for n < 1
 * or K outside 1..FSG_SOLVER_MAX_ITER), 8-byte aligned, in this order with s = K + 1:
 *     double stats_cur[n][32], double lambda[n], double m0[n], double cost[s][n], double lambda_hist[s][n],
 *     float theta_cur[n][6], int32 frozen[n], int32 accepted[s][n], int32 frozen_hist[s][n]
 * rounded up to 8 bytes.  It needs no initialisation: update(0) writes every per-slice field, update(k) row k of the histories.
 * stats_trial (n,32) are the normal equations at theta_trial (n,6), which the call overwrites with the next trial.
 *   cost of a block of sums = [27] / [28].
 *   k = 0   cur <- trial, theta_cur <- theta_trial, m0 = m, lambda = lambda0.  The slice freezes if !(m >= 1), !(sum w > 0)
 *           or any of the 30 sums is not finite.
 *   k >= 1  not frozen: accept iff the 30 trial sums are finite && m_t >= min_overlap * m0 && cost_t < cost_cur.  On accept
 *           cur <- trial, theta_cur <- theta_trial, lambda = max(lambda / factor, lambda_min), and the slice freezes if
 *           cost_old - cost_t <= tol * cost_old.  Otherwise lambda *= factor and the slice freezes once lambda > lambda_max.
 *           A NaN fails every comparison and is rejected.  A frozen slice changes nothing.
 *   next    for k < K and a slice not frozen: A = H + lambda diag(H) from cur (Marquardt's scaling); a parameter with
 *           H_aa == 0 is taken out (unit row and column, g_a = 0, so delta_a = 0); A = L D L^T, Cholesky's factorisation in
 *           its square-root-free form, d_j = A_jj - sum_p (L_jp * L_jp) * d_p, L_rj = (A_rj - sum_p (L_rp * L_jp) * d_p) / d_j,
 *           p increasing; a pivot d_j that is not > 0 freezes the slice; L z = g, z_r /= d_r, L^T x = z, delta = -x;
 *           theta_trial = (float)((double)theta_cur + delta).
 *           A frozen slice, or k = K: theta_trial = theta_cur, so every later launch runs on valid data.
 *   histories, row k: cost[k] = the cost of cur after the decision, lambda_hist[k], accepted[k] (0 for k = 0), frozen_hist[k]
 *           (after the pivot test).
 * Refusals, before any launch and with nothing written: n < 1, K outside 1..FSG_SOLVER_MAX_ITER, k outside 0..K, a null pointer, a short
 * state, !(lambda0 > 0), !(factor > 1), !(lambda_min > 0), !(lambda_max >= lambda_min), !(min_overlap >= 0), !(tol >= 0)
 * (FSG_E_BADARG); state or stats_trial not 8-byte aligned, theta_trial not 4-byte aligned (FSG_E_ALIGN); state, stats_trial
 * and theta_trial sharing a byte (FSG_E_BADARG). */
#define FSG_SVR_SLOTS 32 /* doubles of a slice's row of stats, floats of a tile's partial: the 30 sums and two zeros */
size_t fsg_svr_ws_bytes(int n, int h, int w);
int fsg_svr_normal_f32(const float* transforms, const float* jac, const float* vol, const float* psf, int pd, int ph, int pw,
                       const float* slices, const uint8_t* slices_mask, const float* slices_weight, double* stats, int D, int H,
                       int W, int n, int h, int w, float res_slice, float min_weight, int mode, void* ws, size_t ws_bytes,
                       void* stream);
size_t fsg_svr_state_bytes(int n, int n_iter);
int fsg_svr_update_f32(const double* stats_trial, float* theta_trial, void* state, size_t state_bytes, int n, int k, int n_iter,
                       double lambda0, double factor, double lambda_min, double lambda_max, double min_overlap, double tol,
                       void* stream);

/* ---- grouped registration: several slices share one pose increment (fsg_svr_group.hip) --------------
 * A group of slices (a stack, a package) moves as one rigid body.  Its increment phi = [rotation vector q | translation d] is a
 * rigid motion of the VOLUME frame about the volume centre, x' = Q x + d with [Q | d] = fsg_axisangle2mat_f32(phi).  A slice's
 * matrix [R | t] maps pixel p to the volume-centred point R (p + t), so under the increment
 *     R' = Q R,   t' = t + R'^T d,   dR'/dphi_a = dQ_a R,   dt'/dphi_a = (dQ_a R)^T d + R'^T dd_a
 * with dQ_a, dd_a column a of the (12,6) Jacobian of fsg_axisangle2mat_f32 at phi (fsg_axisangle2mat_backward_f32 on the 12
 * one-hot matrices).  One grouped solve is the launch sequence, for k = 0..K on one stream, G the number of groups:
 *     [Q | d] = axisangle2mat(phi_trial);  its Jacobian;  compose;  fsg_svr_normal_f32 (as it is);  group_reduce;
 *     fsg_svr_update_f32 with n := G on gstats and phi_trial
 * and one compose at the state's theta_cur after the loop.
 *
 * fsg_svr_compose_f32: group_mat (G,12) = [Q | d] row-major 3 x 4, group_jac (G,12,6) row k = d entry k / d phi, base (n,12),
 * group (n) int32 -> transforms (n,12) and jac (n,12,6), the operands of fsg_svr_normal_f32.  One thread per slice and
 * parameter; fp32, one rounding per operation, no contraction, every three-term sum as ((x0 y0) + (x1 y1)) + (x2 y2):
 *     R'[r][c]      = ((Q[r][0] R[0][c]) + (Q[r][1] R[1][c])) + (Q[r][2] R[2][c])
 *     t'[c]         = t[c] + (((R'[0][c] d[0]) + (R'[1][c] d[1])) + (R'[2][c] d[2]))
 *     jac[4r+c][a]  = dR_a[r][c] = ((dQ_a[r][0] R[0][c]) + (dQ_a[r][1] R[1][c])) + (dQ_a[r][2] R[2][c])
 *     jac[4c+3][a]  = (((dR_a[0][c] d[0]) + (dR_a[1][c] d[1])) + (dR_a[2][c] d[2]))
 *                   + (((R'[0][c] dd_a[0]) + (R'[1][c] dd_a[1])) + (R'[2][c] dd_a[2]))
 * with dQ_a[r][m] = group_jac[g][4r+m][a] and dd_a[r] = group_jac[g][4r+3][a].  It holds no pose arithmetic of its own.
 *   group[k] outside [0, G) (-1 by convention) means FIXED: transforms[k] = base[k] bit for bit and jac[k] = 0.  The id is
 *   range-tested before it selects a row and never becomes an address otherwise.
 *   phi = 0: the conversion's small-angle branch gives Q = identity exactly and d = 0, and 1 r + 0 r' + 0 r'' is exact, so
 *   transforms = base bit for bit for finite base (the sign of a zero entry apart: it is the sum's, +0 unless all three
 *   products are -0).  Round 0 of a solve therefore evaluates the poses as given.
 * Refusals, before any launch and with nothing written: a null pointer, n < 1, G < 1 (FSG_E_BADARG); n or G > 65535
 * (FSG_E_TOOBIG); a pointer not 4-byte aligned (FSG_E_ALIGN); transforms or jac sharing a byte with an input or with each
 * other (FSG_E_BADARG).
 *
 * fsg_svr_group_reduce_f64: stats (n,32) DOUBLE, members (n_members) int32 slice indices, offsets (G+1) int32 into members
 * -> gstats (G,32) DOUBLE: gstats[g][k] = stats[members[j]][k] added in double for j = offsets[g] .. offsets[g+1] - 1 in that
 * order from +0.0.  One thread per group and slot; all 32 slots are written; an empty group (offsets[g] == offsets[g+1]) gets
 * zeros; no atomics: a group's row is a pure function of its members' rows, the same bits in any run, on any stream, for any
 * number of other groups.  A member index outside [0, n) adds nothing, and a group whose range is not inside [0, n_members]
 * gets zeros: neither becomes an address.
 * Refusals, before any launch and with nothing written: a null pointer, n < 1, G < 1, n_members < 1 (FSG_E_BADARG); n, G or
 * n_members > 65535 (FSG_E_TOOBIG); stats or gstats not 8-byte aligned, members or offsets not 4-byte aligned (FSG_E_ALIGN);
 * gstats sharing a byte with an input (FSG_E_BADARG). */
int fsg_svr_compose_f32(const float* group_mat, const float* group_jac, const float* base, const int32_t* group, float* transforms,
                        float* jac, int n, int G, void* stream);
int fsg_svr_group_reduce_f64(const double* stats, const int32_t* members, const int32_t* offsets, double* gstats, int n,
                             int n_members, int G, void* stream);

/* ---- outlier weights for the two solves above: robust-statistics EM (fsg_robust.hip) ----------------
 * The W of fsg_cg_* / fsg_svr_normal_f32 from the residual of a reconstruction (Kuklisova-Murgasova et al. 2012): per pixel a
 * Gaussian inlier / uniform outlier posterior p, per slice a two-class mixture over the slice's potential u.  One solve is the
 * launch sequence, T = n_em, all on one stream:
 *     for t = 0..T:  estep(t);  update(t)        then  weights
 * and it is the same sequence whatever the data: nothing returns early, nothing is read back.
 *   y (n,h,w) the acquired slices, s (n,h,w) the simulated ones (A x), fp32; slices_mask (n,h,w) bytes or NULL; sim_weight
 *   (n,h,w) fp32 or NULL, the weight fsg_slice_acq_forward_f32 returns, with min_weight >= 0.
 * Omega: a pixel takes part iff it is inside slices_mask, (with sim_weight) weight > 0 && weight >= min_weight, and
 * e = fl(y - s) is finite.  A NaN or Inf in y, s or the weight therefore leaves the pixel out and reaches no sum.
 *
 * fsg_robust_estep_f32, slot t.  Per pixel of Omega, fp32 with one rounding per operation (no contraction), expf the library's:
 *     e2 = e * e;  x = expf(e2 * inv2var);  p = 1 / (1 + kappa * x), and p = 0 when x overflowed to Inf;  q = 1 - p
 * kappa and inv2var are the two floats update(t - 1) stored; at t == 0, p = 1 and the state is not read.  Per-slice sums: N (the
 * count), sum p, sum p * e2, sum q * q, and min y, max y.  Reduction, no atomics: pixel i of a slice (row-major) belongs to
 * thread (i / 4) mod 256 of workgroup i / 1024 of that slice; a thread adds its four pixels in increasing i from +0; the 64
 * lanes of a wave fold by v[i] += v[i + o], o = 32..1 (shuffle-down; lane 0 holds the sum; min / max by fminf / fmaxf from
 * +Inf / -Inf); the four waves are added in wave order; the workgroup stores one partial of 8 floats (N, sum p, sum p e2,
 * sum q^2, min, max, 0, 0) at ws[slice][workgroup].  ws: DEVICE, 8-byte aligned, fsg_robust_ws_bytes(n, h, w) = 32 bytes per
 * 1024 pixels (rounded up) of every slice; it needs no initialisation.  Loads are 16 bytes per lane when h * w is a multiple
 * of 4, every float pointer is 16-byte aligned and slices_mask 4-byte aligned; scalars otherwise, same values and same sums.
 *
 * fsg_robust_update_f32, slot t: one workgroup, double arithmetic.  A slice's row = its partials added in DOUBLE in workgroup
 * order from +0.0 (min / max by fmin / fmax; a slice without a pixel stores min = max = 0).  Given kappa and inv2var a row is a
 * pure function of that slice's data.  ok_k = N_k >= min_pixels && N_k > 0; a slice that is not ok has ws = 0 in every slot.
 *   t == 0     R = max y - min y over Omega, m = 1 / R, sigma_min = sigma_floor * R: the constants of the solve.
 *   pixels     w_k = ws[t-1][k] (1 at t == 0; 0 for a slice not ok); over the slices in index order from +0.0:
 *              S0 = sum w_k * sum p, S2 = sum w_k * sum p e2, Nw = sum w_k * N_k;
 *              var = max(S2 / S0, sigma_min^2);  c = S0 / Nw, and c = c0 at t == 0;
 *              kappa = (float)(((1 - c) / c) * m * sqrt(2 pi var));  inv2var = (float)(1 / (2 var)).
 *   slices     t >= 1, one sweep over u_k = sqrt(sum q^2 / N_k) of the ok slices, sums in index order, w the OLD weights:
 *              sw = sum w, mu1 = sum w u / sw, v1 = max(sum w (u - mu1)^2 / sw, slice_floor^2);  so = sum (1 - w);
 *              so > 0: mu2 = sum (1 - w) u / so, v2 = sum (1 - w)(u - mu2)^2 / so;  else mu2 = (max u + mu1) / 2, v2 = 0;
 *              !(v2 > 0): v2 = (mu2 - mu1)^2 / 4;  v2 = max(v2, slice_floor^2);  mix = sw / n_ok;
 *              ws[t][k] = 1 if u < mu1, 0 if u > mu2, else g1 mix / (g1 mix + g2 (1 - mix)), g the normal densities of u under
 *              (mu1, v1) and (mu2, v2); where that quotient is not a number (both densities underflowed, a zero variance) the
 *              class of the nearer mean.  At t == 0, ws[0][k] = 1.
 *   freeze     R == 0 or not finite, Nw == 0, S0 == 0, var == 0 or any scalar above not finite: the solve is frozen from this
 *              slot on.  Frozen: ws[t][k] = 1 for every ok slice, kappa = inv2var = 0 (so p = 1), sigma, c, mu1, mu2 of the
 *              slot are 0, frozen[t] = 1, and every later slot repeats this.  No NaN is ever stored.
 * state: one DEVICE block of fsg_robust_state_bytes(n, T) bytes (0 for n < 1 or T outside 1..FSG_SOLVER_MAX_ITER), 8-byte aligned, in this
 * order with s = T + 1:
 *     double consts[4] (R, m, sigma_min, 0), double rows[n][6] (N, sum p, sum p e2, sum q^2, min y, max y: the LAST estep's),
 *     double u[n], double sigma[s], double c[s], double mu1[s], double mu2[s], double ws[s][n], float kappa, float inv2var,
 *     int32 frozen[s]
 * rounded up to 8 bytes.  It needs no initialisation: update(0) writes the constants, update(t) every per-slice field and
 * slot t of the histories; a launch reads only what an EARLIER launch wrote.
 *
 * fsg_robust_weights_f32: out (n,h,w) fp32 = (float)ws[T][k] on Omega and 0 elsewhere (FSG_ROBUST_SLICE), or
 * fl((float)ws[T][k] * p) with p under the kappa and inv2var update(T) stored (FSG_ROBUST_BOTH).
 *
 * Determinism: no atomics and every order fixed, so the same bits in any run and on any stream.  sigma and c are GLOBAL sums
 * in slice-index order, so permuting the slices permutes the result only up to rounding (unlike fsg_svr_normal_f32, whose
 * rows do not see the other slices).
 * Refusals, all before any launch and with nothing written: n, h or w < 1, T outside 1..FSG_SOLVER_MAX_ITER, t outside 0..T, a null y, s,
 * state, ws or out, a short state or ws, min_weight negative or NaN, c0 outside (0, 1] or NaN, sigma_floor or slice_floor
 * negative, NaN or Inf, min_pixels < 0, an unknown level (FSG_E_BADARG); n > 65535, n * h * w > 2^31 - 1 or
 * h * w > 2^31 - 1 - 1024 (a slice's pixels are counted in int, 1024 to a workgroup; FSG_E_TOOBIG, and fsg_robust_ws_bytes
 * returns 0 for the same sizes);
 * state or ws not 8-byte aligned, a float pointer not 4-byte aligned (FSG_E_ALIGN); ws sharing a byte with an input or the
 * state, out sharing a byte with an input or the state (FSG_E_BADARG). */
#define FSG_ROBUST_SLICE 0
#define FSG_ROBUST_BOTH 1
#define FSG_ROBUST_ROW 6 /* doubles of a slice's entry of rows[n][6] in the state */
size_t fsg_robust_ws_bytes(int n, int h, int w);
size_t fsg_robust_state_bytes(int n, int n_em);
int fsg_robust_estep_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                         int n, int h, int w, int t, int n_em, const void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                         void* stream);
int fsg_robust_update_f32(void* state, size_t state_bytes, const void* ws, size_t ws_bytes, int n, int h, int w, int t, int n_em,
                          double c0, double sigma_floor, double slice_floor, int min_pixels, void* stream);
int fsg_robust_weights_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                           int n, int h, int w, int n_em, int level, const void* state, size_t state_bytes, float* out,
                           void* stream);

/* ---- slice intensity matching for the reconstruction: per-slice scale and smooth bias field (fsg_imatch.hip; DESIGN.md
 * section 28) ----------------------------------------------------------------------------------------------------------------
 * The third part of the slice-to-volume method (Kuklisova-Murgasova et al. 2012) beside the solve and the robust statistics:
 * every acquired slice gets one multiplicative scale and one smooth multiplicative bias field exp(bias), both estimated from the
 * slice and its simulation s = A x and both removed before the next solve.  One matching is the launch sequence, on one stream:
 *     sums;  scale;  (sigma > 0: bias = three launches, rows, columns, means;)  apply
 * and it is the same sequence whatever the data: nothing returns early, nothing is read back.
 *   y (n,h,w) the acquired slices, s (n,h,w) the simulated ones, fp32; slices_mask (n,h,w) bytes or NULL; sim_weight (n,h,w) fp32
 *   or NULL with min_weight >= 0, as fsg_robust_*; pix_weight (n,h,w) fp32 or NULL, the robust weights omega (NULL: omega = 1);
 *   bias0 (n,h,w) fp32 or NULL, the log-bias carried from an earlier matching (NULL: 0); sigma, a double, in pixels.
 * c = fl(expf(-bias0) * y), and c = y without bias0: the slice with the carried bias removed.
 * Omega: a pixel takes part iff it is inside slices_mask, (with sim_weight) weight > 0 && weight >= min_weight, y, s and c are
 * finite, and (with pix_weight) omega is finite and > 0.  A NaN or Inf in any array leaves the pixel out and reaches no sum.
 *
 * fsg_imatch_sums_f32.  Per pixel of Omega, fp32 with one rounding per operation (no contraction), expf the library's:
 *     t = fl(omega * c) (t = c without pix_weight);  the terms 1, fl(t * s), fl(t * c)
 * Per-slice sums: N (the count), A = sum omega c s, B = sum omega c c, and min y, max y.  Reduction exactly as
 * fsg_robust_estep_f32: pixel i of a slice belongs to thread (i / 4) mod 256 of workgroup i / 1024 of that slice; a thread adds
 * its four pixels in increasing i from +0; the 64 lanes of a wave fold by v[i] += v[i + o], o = 32..1 (shuffle-down; min / max by
 * fminf / fmaxf from +Inf / -Inf); the four waves are added in wave order; the workgroup stores one partial of 8 floats (N, A, B,
 * min, max, 0, 0, 0) at ws[slice][workgroup].  Loads are 16 bytes per lane when h * w is a multiple of 4, every float pointer is
 * 16-byte aligned and slices_mask 4-byte aligned; scalars otherwise, same values and same sums.
 *
 * fsg_imatch_scale_f32: one workgroup, double arithmetic.  A slice's row = its partials added in DOUBLE in workgroup order from
 * +0.0 (min / max by fmin / fmax; a slice without a pixel stores min = max = 0): rows[k] = (N, A, B, min y, max y).
 *     R = max y - min y over all of Omega;  floor = log_floor * R
 *     own_k = N_k >= min_pixels && N_k > 0 && A_k, B_k finite and > 0 && A_k / B_k finite;  raw_k = A_k / B_k (0 for a slice
 *         that is not own_k; its A and B are stored as 0 when either is not finite): the least-squares gain that takes c to s,
 *         the minimiser of sum omega (raw c - s)^2
 *     gauge: g = (sum of raw_k over the own_k slices in index order from +0.0) / (their number): a common gain of all slices is
 *         the volume's, not a slice's, so the scales have arithmetic mean 1 over the slices that have one
 *     scale_k = (float)(raw_k / g);  a slice that is not own_k keeps scale_k = 1
 *     freeze: R == 0 or not finite, no slice own_k, g not finite or not > 0, or a scale_k that is not finite or not > 0:
 *         frozen = 1, every scale_k = 1 and every ok_k = 0.  Otherwise ok_k = own_k.  No NaN is ever stored.
 *     mean_k = 0 (fsg_imatch_bias_f32 overwrites it).
 * A slice with ok_k == 0 keeps scale 1 and its bias as given, in every later launch.
 *
 * fsg_imatch_bias_f32, only for sigma > 0 (sigma == 0 is scale only: the entry is not called and refuses).  Rr = ceil(3 sigma),
 * taps g[t] = (float)exp(-(t * t) / (2 sigma^2)), t = 0..Rr, computed on the host in double and NOT normalised: only a quotient
 * of two sums under the same taps is formed.
 *   Omega_b: a pixel of Omega whose slice is ok, with d = fl(scale_k * c) > (float)floor and s > (float)floor.
 *   r = logf(fl(d / s)) (the division correctly rounded, logf the library's); a pixel whose r is not finite is not in Omega_b.
 *   Planes: P = fl(omega * r) and Q = omega on Omega_b (r and 1 without pix_weight), 0 elsewhere.
 *   rows     for both planes, per pixel (row i, column j): acc = +0; for t = -Rr..Rr in increasing t, the taps with
 *            0 <= j + t < w only (a tap outside the slice is skipped; one inside the slice and outside Omega_b runs with its
 *            zero): acc = fmaf(g[|t|], plane[i][j + t], acc).  -> P1, Q1.
 *   columns  the same along i over P1 and Q1: t = -Rr..Rr increasing, 0 <= i + t < h, acc = fmaf(g[|t|], plane1[i + t][j], acc),
 *            from +0.  -> P2, Q2.  inc = Q2 >= FLT_MIN ? fl(P2 / Q2) : 0;  b1 = fl(bias0 + inc) (b1 = inc without bias0),
 *            written to `bias`.  A pixel all of whose taps miss Omega_b has Q2 == 0 and inc == 0 exactly.
 *   means    per ok slice m_k = sum over Omega_b of fl(omega * b1) / sum over Omega_b of omega (0 when the denominator is 0, and
 *            for a slice that is not ok): a thread of the column pass adds its pixels in increasing row from +0, the 256 threads
 *            of a tile fold as in fsg_svr_normal_f32 (shuffle-down, waves in order), one partial of two floats per tile at
 *            ws[slice][tile], tile = tile_y * tiles_x + tile_x, tiles of 64 rows by 32 columns; the third launch adds a slice's
 *            partials in DOUBLE in tile order from +0.0 and stores mean_k.  The smooth field takes no part of the scale's work.
 *   planes: DEVICE workspace of fsg_imatch_plane_bytes(n, h, w) = 12 bytes a pixel (P1, Q1 and Q, each (n,h,w) fp32), 16-byte
 *   aligned; it needs no initialisation.
 *
 * fsg_imatch_apply_f32.  mode FSG_IMATCH_WITH_BIAS: `bias` holds b1; bias = fl(b1 - (float)mean_k) on every pixel of an ok
 * slice, b1 unchanged on the others.  mode FSG_IMATCH_SCALE_ONLY: bias = bias0, or 0 without it.  Then on EVERY pixel
 *     corrected = fl(scale_k * fl(expf(-bias) * y))
 * so a NaN in y stays a NaN in corrected, at that pixel only.  16-byte loads and stores as above.
 *
 * state: one DEVICE block of fsg_imatch_state_bytes(n) bytes (0 for n < 1 or n > 65535), 8-byte aligned, in this order:
 *     double consts[4] (R, floor, g, the number of ok slices), double rows[n][5] (N, A, B, min y, max y), double raw[n],
 *     double mean[n], float scale[n], int32 ok[n], int32 frozen
 * rounded up to 8 bytes.  It needs no initialisation: scale writes every field, bias overwrites mean; a launch reads only what
 * an EARLIER launch wrote.  ws: DEVICE, 8-byte aligned, fsg_imatch_ws_bytes(n, h, w) = 32 bytes per 1024 pixels (rounded up) of
 * every slice for the sums, followed by 8 bytes per tile of every slice for the means; it needs no initialisation.
 *
 * Determinism: no atomics and every order fixed, so the same bits in any run and on any stream.  A slice's row is a function of
 * that slice alone; R, g and so every scale are GLOBAL sums in slice-index order (as sigma and c of fsg_robust_*).
 * Refusals, all before any launch and with nothing written: n, h or w < 1, a null y, s, state, ws, planes, bias or corrected, a
 * short state, ws or plane buffer, min_weight or log_floor negative or NaN (log_floor Inf too), min_pixels < 0, sigma negative,
 * NaN, Inf or 0 in fsg_imatch_bias_f32, 3 sigma > FSG_IMATCH_MAX_RADIUS, an unknown mode (FSG_E_BADARG); n > 65535,
 * n * h * w > 2^31 - 1, h * w > 2^31 - 1 - 1024 (a slice's pixels are counted in int, 1024 to a workgroup), or h > 65535 in
 * fsg_imatch_bias_f32 (FSG_E_TOOBIG; the three fsg_imatch_*_bytes return 0 for the same sizes); state or ws not 8-byte aligned, planes not 16-byte aligned, a float pointer not 4-byte
 * aligned (FSG_E_ALIGN); an output, the planes, ws or the state sharing a byte with an input or with one another (FSG_E_BADARG;
 * `bias` of apply is in place by contract). */
#define FSG_IMATCH_SCALE_ONLY 0
#define FSG_IMATCH_WITH_BIAS 1
#define FSG_IMATCH_ROW 5         /* doubles of a slice's entry of rows[n][5] in the state */
#define FSG_IMATCH_MAX_RADIUS 48 /* the largest ceil(3 sigma): sigma up to 16 pixels, 12 mm at 0.75 mm */
size_t fsg_imatch_ws_bytes(int n, int h, int w);
size_t fsg_imatch_state_bytes(int n);
size_t fsg_imatch_plane_bytes(int n, int h, int w);
int fsg_imatch_sums_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                        const float* pix_weight, const float* bias0, int n, int h, int w, void* ws, size_t ws_bytes,
                        void* stream);
int fsg_imatch_scale_f32(void* state, size_t state_bytes, const void* ws, size_t ws_bytes, int n, int h, int w, double log_floor,
                         int min_pixels, void* stream);
int fsg_imatch_bias_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                        const float* pix_weight, const float* bias0, double sigma, int n, int h, int w, void* state,
                        size_t state_bytes, void* planes, size_t plane_bytes, void* ws, size_t ws_bytes, float* bias,
                        void* stream);
int fsg_imatch_apply_f32(const float* y, const float* bias0, int mode, int n, int h, int w, const void* state,
                         size_t state_bytes, float* bias, float* corrected, void* stream);

/* ---- SR-artifact volumetric helpers, fsg_artifacts.hip ------------------------------------ */
/* out = clamp(sum_g exp(-(((x-c0)/s0)^2 + ((y-c1)/s1)^2 + ((z-c2)/s2)^2) / 2), 0, 1) over a (D,H,W) grid with
 * x the LAST axis -- generator/artifacts/utils.py:125-160 `mog_3d_tensor`, including its convention that a
 * centre is unpacked as (x0,y0,z0) (callers pass first-axis indices first: the reference's own transposition).
 * centers, sigmas: DEVICE (k,3) fp32.  tables: caller-owned workspace of k*3*max(D,H,W) floats. */
int fsg_mog3d_f32(const float* centers, const float* sigmas, int k, int D, int H, int W, float* tables, float* out,
                  void* stream);
/* Raw fractal Perlin noise sum_q amps[q] * perlin_q (generator/artifacts/utils.py:224-384) on an (n0,n1,n2) grid and
 * its min / max (ordered keys, mm[0], mm[1]; caller initialises with fsg_minmax_init(mm,1,1)).  Per octave q:
 * grads[q] DEVICE (r0+1,r1+1,r2+1,3) unit gradients (tileable wrap already applied), lins[q] DEVICE
 * linspace(0,r_a,n_a) for the three axes back to back, res[3q..3q+2] = (r0,r1,r2).  grads/lins/res/amps: HOST arrays. */
int fsg_perlin_fractal_f32(const float* const* grads, const float* const* lins, const int32_t* res, const float* amps,
                           int noct, int n0, int n1, int n2, float* out, int32_t* mm, void* stream);
/* out = (1 - w) a + w b, the spatially weighted merge of simulate_reco.py:704, augmentation/artifacts.py:125, :337.
 *   w_mode 0: w is the weight volume; 1: w is raw Perlin noise, normalised on the fly as
 *             clamp((w + increase - min) / (max - min), 0, 1) with w_mm from fsg_perlin_fractal_f32 (utils.py:386-387);
 *   seg != NULL: w *= (seg > 0)                                              (artifacts.py:336-337);
 *   b_mode 1: b is the multi-scale noise field, b' = clamp(a + std * b / max|b|, 0, 2 max a) with b_mm / a_mm the
 *             min/max keys of b and a                                        (artifacts.py:322-327).
 * out may be NULL (then only w_out, the weight actually used, is written); w_out may be NULL. */
int fsg_blend_f32(const float* a, const float* b, const float* w, size_t n, int w_mode, const int32_t* w_mm, float increase,
                  const float* seg, int b_mode, const int32_t* b_mm, const int32_t* a_mm, float std, float* out,
                  float* w_out, void* stream);
/* Scanner.add_noise (simulate_reco.py:236-256), in place: s = sqrt((s + sigma z1)^2 + (sigma z2)^2) where s > threshold.
 * noise1/noise2 dense fields (host-tape mode) or both NULL: Philox(seed, stream_id), two normals per pixel. */
int fsg_slice_noise_f32(float* slices, size_t n, float threshold, float sigma, const float* noise1, const float* noise2,
                        uint64_t seed, uint64_t stream_id, void* stream);
/* Scanner.signal_void (simulate_reco.py:258-298), in place on the nvoid slices slice_ids[t]:
 * s *= 1 - A exp(sx x'^2 + sy y'^2); params (nvoid,7) = {yc, xc, cos, sin, A, sx, sy}; ylin (h), xlin (w).
 * slice_ids must be DISTINCT and inside the stack: every void has a workgroup row of its own, two voids naming one slice
 * race, and the ids are on the device, where this call cannot look at them.  kernels.slice_void_ checks them on the host. */
int fsg_slice_void_f32(float* slices, int h, int w, const int32_t* slice_ids, const float* params, int nvoid,
                       const float* ylin, const float* xlin, void* stream);
/* sums[i] = sum of slice i (simulate_reco.py:409), deterministic. */
int fsg_slice_sums_f32(const float* slices, int n, size_t hw, float* sums, void* stream);

/* The reference picks random voxels of a mask as `torch.where(mask)` + `torch.randperm(count)[:k]`
 * (simulate_reco.py:661-664, augmentation/artifacts.py:110-113, :199-202, :565-567), materialising three int64 index
 * lists of the whole mask.  Here: per-bucket counts (buckets of FSG_NZ_BUCKET = 4096 voxels, raster order), a host
 * prefix sum, then the flat index of the rank[q]-th voxel of bucket[q] satisfying the predicate for each request
 * (-1 if the bucket holds fewer).  Predicate on (float)v: mode 0: v > value, 1: v == value, 2: v != value. */
#define FSG_NZ_BUCKET 4096
int fsg_nonzero_count_f32(const float* v, size_t n, int mode, float value, int32_t* counts, void* stream);
int fsg_nonzero_count_u8(const uint8_t* v, size_t n, int mode, float value, int32_t* counts, void* stream);
int fsg_nonzero_select_f32(const float* v, size_t n, int mode, float value, const int32_t* bucket, const int32_t* rank,
                           int nreq, long long* out, void* stream);
int fsg_nonzero_select_u8(const uint8_t* v, size_t n, int mode, float value, const int32_t* bucket, const int32_t* rank,
                          int nreq, long long* out, void* stream);

/* Weighted random voxel picks without a host pass over the mask (keyed mode's picks of the SR-artifact stages).
 * A voxel is ELIGIBLE when `pred` satisfies the predicate (mode / value as for fsg_nonzero_count_*) and its weight is > 0
 * (weight: DEVICE float32, n elements, NaN and negative count as 0; NULL = 1 per voxel).  S_e = inclusive float64 prefix sum
 * of the weights over the eligible voxels in raster order, total = the last S_e.  Candidate q (q < m) is the first eligible
 * voxel with S_e > u[q] * total (product in float64; u: DEVICE, m doubles in [0,1)); the last eligible voxel if rounding
 * leaves none.  out (DEVICE, k + 2 int64): out[0] = eligible voxels, out[1] = found = distinct picks (<= k),
 * out[2 .. 2+found) = flat indices of the first k distinct candidates in candidate order, the rest -1.  Nothing eligible:
 * out[0] = out[1] = 0 and all -1; n == 0 the same with one launch that writes `out` (pred, weight, ws may be NULL).
 * 1 <= k <= m, m <= 4096, k <= 1024: FSG_E_BADARG (k > m, k or m < 1) / FSG_E_TOOBIG otherwise, `out` untouched.
 * The float64 sums are taken in a fixed order (lane quads, a wave scan per 256 voxels, chunks, buckets of FSG_NZ_BUCKET,
 * segments of buckets) with no floating-point atomics: the same inputs give the same `out` bit for bit; where the sums
 * are exact the result is the exact-arithmetic one, otherwise it may differ from a sequential float64 sum only for a
 * u[q] * total within 2^-40 total of a prefix boundary.  ws: DEVICE scratch, 16-byte aligned, >= fsg_voxel_pick_ws_bytes(n).
 * Four launches, no host synchronisation. */
size_t fsg_voxel_pick_ws_bytes(size_t n);
int fsg_voxel_pick_f32(const float* pred, size_t n, int mode, float value, const float* weight, const double* u, int m, int k,
                       long long* out, void* ws, size_t ws_bytes, void* stream);
int fsg_voxel_pick_u8(const uint8_t* pred, size_t n, int mode, float value, const float* weight, const double* u, int m, int k,
                      long long* out, void* ws, size_t ws_bytes, void* stream);

/* out[offsets[b] + r] = values[e] for the r-th voxel e of bucket b with `pred[e]` satisfying the predicate: the
 * boolean-mask gather `values[mask]` (augmentation/artifacts.py:78-80) in raster order; offsets = exclusive prefix sum
 * of fsg_nonzero_count_f32's counts (DEVICE, int64). */
int fsg_compact_f32(const float* values, const float* pred, size_t n, int mode, float value, const long long* offsets,
                    float* out, void* stream);
/* Element-wise glue of the artifact stages.  op 0: a + b; 1: (a > value) as 0/1; 2: (a == value) as 0/1; 3: a * b;
 * 4: a * (b > value); 5: max(a, b); 6: ((a - b) > value) as 0/1; 7: (a <= value) as 0/1.  b may be NULL for ops 1, 2, 7. */
int fsg_ewise_f32(const float* a, const float* b, size_t n, int op, float value, float* out, void* stream);

/* One axis pass of a capped distance transform: dst[v] = min over |t| <= radius (inside the volume) of
 * src'[v + t e_axis] + cost(t), cost = t^2 (metric 0) or |t| (metric 1); first != 0: src is a mask (set -> 0, else 1e9).
 * Passes over axes 0,1,2 give the squared Euclidean / city-block distance to the mask where it is <= radius^2 / radius:
 * `dist <= radius^2` is the reference's zero-padded conv3d with skimage's ball(radius) > 0 (augmentation/artifacts.py:484-499)
 * without its (2r+1)^3 taps; `city-block dist <= k` is k successive ball(1) dilations (artifacts.py:587-589).  src != dst. */
int fsg_dist_pass_f32(const float* src, float* dst, int n0, int n1, int n2, int axis, int radius, int metric, int first,
                      void* stream);
/* SimulatedBoundaries' fuzzy mask (augmentation/artifacts.py:565-604) fused: k = clamp(rint(p n_dilate - 1), 0) with
 * p = mog where mask_modif added voxels to mask (0 elsewhere); m = mask_modif * (dist <= max(k-1, 0)), dist = city-block
 * distance to mask; out = image * m (out/image may be NULL), mask_out = m (may be NULL).
 * p n_dilate - 1 is two float32 roundings, as in the reference (the library is built with -ffp-contract=off: no fused
 * multiply-add), and rint rounds ties to even. */
int fsg_boundary_mask_f32(const float* image, const float* mask, const float* mask_modif, const float* mog, const float* dist,
                          int n_dilate, size_t n, float* out, float* mask_out, void* stream);
/* out = a * (u < p), u ~ U[0,1) from Philox(seed, stream_id) per element: device-RNG thinning of a voxel set. */
int fsg_bernoulli_keep_f32(const float* a, size_t n, float p, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* out[idx[q]] = value for q < k (idx DEVICE int64; entries outside [0, n) are skipped). */
int fsg_scatter_const_f32(float* out, size_t n, const long long* idx, int k, float value, void* stream);

/* ---- whole-sample launch sequence -------------------------------------------------------------------------- */
/* One call = the fused kernel sequence of FetalSynthGen.sample (generator/model.py:231-276) for the
 * seeds-based path: GMM draw -> [rows, margins, warp(+gamma+bias, labels)] -> [blur x,y,z, resample+noise,
 * zoom-back min/max, zoom-back+normalise] on `stream`.  All random quantities are inputs (drawn by the host in
 * the reference's order).  Workspaces are caller-owned and may be reused by the next call on the same stream.
 * Returns FSG_E_ALIGN / FSG_E_TOOBIG for configurations the fused kernels do not cover (the caller then issues
 * the entry points above one by one). */
/* Head of a sample as ONE launch: the GMM draw (as fsg_gmm_sample_u8x4), the per-row coarse values (as
 * fsg_deform_rows_f32) and the six-face pass of fsg_coords_floormin_f32 share no data, so their workgroups run side by side.
 * mm3 must already hold initialised keys (fsg_minmax_init, or key values uploaded with the parameters): nothing in this
 * launch resets them.  fsg_coords_floormin_rest_f32 is the conditional full pass that completes the floor(min) keys. */
int fsg_sample_head_f32(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                        const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                        uint64_t stream_id, float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                        int row_stride, int32_t* mm3, void* stream);
int fsg_coords_floormin_rest_f32(const fsg_deform* d, int32_t* mm3, void* stream);
/* The same launch with the seed labels of a subject as ONE uint16 code volume instead of four uint8 volumes (6 instead of 8
 * bytes per voxel): codes[v] indexes `tuples`, ntuples rows of `stride` bytes, row c = the value every seed volume of the
 * subject holds at the voxels with code c (built once per subject by the caller: the distinct columns of the stacked seed
 * volumes); sel[m] = the byte of a row that belongs to the volume selected for meta label m (a zero byte for an absent one).
 * label = (tuples[c][sel[0]] + .. + tuples[c][sel[3]]) & 255 -- what fsg_sample_head_f32 adds up voxel by voxel
 * (rand_gmm.py:91-99) -- so the output is bit-identical.  n % 8 == 0, n <= 2^30, ntuples <= FSG_CODES_MAX, Philox noise only;
 * otherwise FSG_E_ALIGN / FSG_E_TOOBIG and the caller uses fsg_sample_head_f32.  (One-byte codes for subjects with <= 256
 * columns were measured and dropped: the kernel follows the width of a wave's read request, not its bytes -- 35.1 / 33.0 / 38.3 us
 * with 4 / 8 / 16-byte loads of uint8 codes against 31.6 / 30.8 with 8 / 16-byte loads of uint16 codes.) */
#define FSG_CODES_MAX 2048
int fsg_sample_head_codes_f32(const uint16_t* codes, const uint8_t* tuples, int ntuples, int stride, const int32_t sel[4],
                              size_t n, const float* mus, const float* sigmas, int ntab, uint64_t seed, uint64_t stream_id,
                              float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows, int row_stride,
                              int32_t* mm3, void* stream);

/* Builds codes (n uint16) and tuples (cap rows of `stride` bytes; row c, byte j = the value of parts[j] at the voxels with code
 * c; bytes >= nparts stay 0) from the nparts <= 64 uint8 volumes of a subject in one pass (csrc/fsg_codes.hip).  parts: HOST
 * array of device pointers.  work: fsg_seed_codes_work_bytes() of device scratch (16-byte aligned).  *count_dev receives the
 * number of distinct columns: usable only if it is <= cap (<= FSG_CODES_MAX) -- read it after synchronising.  The numbering of
 * the codes depends on the order in which the lanes met the columns (run to run); codes and tuples are consistent with each
 * other, which is all fsg_sample_head_codes_f32 needs.  No reference counterpart: the reference re-reads and adds up the four
 * selected NIfTI volumes per sample (rand_gmm.py:91-99). */
size_t fsg_seed_codes_work_bytes(void);
int fsg_seed_codes_build(const uint8_t* const* parts, int nparts, size_t n, int stride, uint16_t* codes, uint8_t* tuples, int cap,
                         void* work, size_t work_bytes, int32_t* count_dev, void* stream);

typedef struct fsg_sample_plan {
  int32_t shape[3];
  /* K1 */
  const uint8_t* label_parts[4]; /* per-meta-label seed volumes (disjoint supports), [1..3] may be NULL      */
  const float* mus;
  const float* sigmas;
  int32_t ntab;
  const float* gmm_noise;        /* NULL: Philox(gmm_seed, gmm_stream)                                       */
  uint64_t gmm_seed, gmm_stream;
  /* K2..K5 */
  int32_t deform_active;
  fsg_deform deform;             /* rows / row_stride are filled in by the call                              */
  const float* seg_in;           /* float32 label volume and its deformed copy (deform_active only)          */
  float* seg_out;
  fsg_epilogue epi;              /* gamma <= 0: off; bias NULL: off (applied stand-alone when not deforming)  */
  /* K6..K8 */
  int32_t resample_active;
  int32_t low_shape[3];
  const fsg_tap* rs_tab[3];      /* full -> low resolution tables                                            */
  const fsg_tap* back_tab[3];    /* low -> full resolution tables                                            */
  int32_t blur_ntaps[3];         /* 0: axis not blurred                                                      */
  float blur_taps[3][129];
  int32_t noise_mode;            /* 0 none, 1 `noise` pointer, 2 Philox(noise_seed, noise_stream)            */
  const float* noise;
  uint64_t noise_seed, noise_stream;
  float noise_std;
  /* K9/K10 */
  int32_t scale01;               /* 1: also apply the dataset's [0,1] scaling (data/datasets.py:311)         */
  /* workspaces + result */
  float* ws0;                    /* shape[] floats each                                                       */
  float* ws1;
  float* ws_low;                 /* >= prod(low_shape) floats                                                 */
  float* ws_rows;                /* shape[0]*shape[1]*row_stride floats, or NULL                              */
  int32_t row_stride;
  int32_t* mm8;                  /* 8 x int32                                                                 */
  int32_t mm8_preset;            /* 1: the keys already hold [+inf x4 | -inf x4] (uploaded with the parameters): no reset
                                  *    launch-side, and the head of the sample runs as one launch (fsg_sample_head_f32)  */
  float* out;                    /* shape[] floats                                                            */
  void* ev_blur_begin;           /* optional hipEvent_t pair recorded around the blur passes (fsg_event_*)     */
  void* ev_blur_end;
  int32_t* mm_slots;             /* optional: mm_nslots initialised slots (see fsg_zoom3d_minmax_sharded_f32) for the min / max
                                    of the zoom-back; the [0,1] scaling then reads them instead of mm8[3..4] */
  int32_t mm_nslots;
  const uint8_t* seg_in_u8;      /* optional uint8 copy of seg_in (same values): the label gather then reads 1 B/voxel
                                    (fsg_warp_f32_u8_to_f32); seg_in stays required as the fallback source */
  /* parameter upload as part of the call (optional): arena_bytes (multiple of 16) from the device-visible pinned block
   * arena_host to arena_dev -- the block every pointer above with small per-sample content points into -- before the first
   * kernel.  The caller must not reuse arena_host before work enqueued on `stream` AFTER this call has completed. */
  const void* arena_host;
  void* arena_dev;
  uint64_t arena_bytes;
  /* overlap / ws_seq: retired (a side stream for the upload and the head of the sample, measured slower and removed).
   * Ignored: results are those of overlap == 0, and the layout stays.  Never reuse them. */
  int32_t overlap;
  uint64_t ws_seq;
  /* optional: the deformed labels as uint8 (needs seg_in_u8; seg_out may then be NULL): the device-resident streaming hand-over
   * (reference data/datasets.py:315-323 converts the labels after the fact) without a conversion pass */
  uint8_t* seg_out_u8;
  /* optional stage trace (measurement only): trace_events = trace_cap hipEvent_t handles (fsg_event_create), trace_ids =
   * trace_cap + 1 ints.  An event is recorded before the first launch (id FSG_ST_BEGIN) and after every launch of the
   * sample (id = the FSG_ST_* of that launch); trace_ids[trace_cap] receives the number of events recorded.  The time
   * between two consecutive events is the later one's launch plus one barrier packet (each record is one). */
  void** trace_events;
  int32_t* trace_ids;
  int32_t trace_cap;
  int32_t trace_start;           /* events the caller has already recorded (fsg_keyed_sample_run: 1, the one before its draw
                                  * kernel); the first event of this call then carries trace_first_id instead of FSG_ST_BEGIN */
  int32_t trace_first_id;
  /* optional (ABI 3): the subject's seed labels as one code volume (fsg_sample_head_codes_f32); label_parts stay valid and are
   * what every path without the one-launch head reads */
  const uint16_t* label_codes;
  const uint8_t* code_tuples;
  int32_t code_ntuples, code_stride;
  int32_t code_sel[4];
  /* Look-ahead (ABI 3; set by fsg_keyed_sample_run when the caller names the next sample, zero otherwise): the keyed draw job
   * of the NEXT sample -- it depends on nothing of this one -- goes out beside this sample's one-launch head
   * instead of as a launch of its own (a job of more than 4096 workgroups is not carried).  ride_draw: host pointer to a library-internal argument block, valid for the call.
   * *rode (may be NULL) receives 1 when the job really went out. */
  const void* ride_draw;
  uint32_t ride_draw_blocks;
  int32_t* rode;
} fsg_sample_plan;
enum {
  FSG_ST_BEGIN = 0, FSG_ST_UPLOAD = 1, FSG_ST_DRAW = 2, FSG_ST_HEAD = 3, FSG_ST_FLOORMIN = 4, FSG_ST_WARP = 5, FSG_ST_BLUR_X = 6,
  FSG_ST_BLUR_Y = 7, FSG_ST_BLUR_Z = 8, FSG_ST_BLUR_YZ = 9, FSG_ST_K7 = 10, FSG_ST_K9A = 11, FSG_ST_K9B = 12, FSG_ST_GMM = 13,
  FSG_ST_ROWS = 14, FSG_ST_POINTWISE = 15, FSG_ST_BLUR_RS_X = 16, FSG_ST_BLUR_RS_YZ = 17, FSG_ST_COUNT = 18
};
int fsg_sample_run(const fsg_sample_plan* plan_host, void* stream);
/* Real-image samples (ABI 4): the volumes of a sample that carries an image, beside its plan.  They live in a struct of their
 * own, not at the end of fsg_sample_plan: the plan and its flat form (FSG_PLAN_I_*, one slot per field) keep their layout.
 * All three optional.
 * prior_in: a float32 volume of shape[] that REPLACES the GMM draw (the reference's image-as-intensity prior, model.py:138:
 *   the subject's image scaled to 0..255 -- a constant of the subject, computed by the caller once).  The plan's label_parts, mus,
 *   sigmas and code volume are then not read and may be NULL / 0; the rows and faces jobs of the one-launch head stay.  Never
 *   written: gamma and the bias field run on it as they do on the GMM volume when no deformation is drawn.
 * image_in / image_out: the raw image (float32, shape[]) and its deformed copy, written by the SAME warp launch as out and the
 *   labels (fsg_warp_dual_f32; two launches where that declines).  deform_active only: without a deformation image_out is not
 *   written and the caller passes the image through, as it does with the labels.  image_in without image_out: FSG_E_BADARG,
 *   nothing launched.
 * fsg_sample_run_image(plan, NULL, stream) is fsg_sample_run(plan, stream). */
typedef struct fsg_sample_image {
  const float* image_in;
  float* image_out;
  const float* prior_in;
} fsg_sample_image;
int fsg_sample_run_image(const fsg_sample_plan* plan_host, const fsg_sample_image* image_host, void* stream);
/* Layout check for FFI mirrors of the structs: which = FSG_SIZEOF_x -> sizeof(fsg_x) (0: fsg_sample_plan, 6 .. 10: fsg_tap,
 * fsg_deform, fsg_epilogue, fsg_keyed_config, fsg_keyed_draws; 12: fsg_sample_image; 13: fsg_keyed_overrides); 1 / 2 / 3 / 4 / 5 -> offsetof blur_taps /
 * out / seg_in_u8 / ws_seq / code_sel in fsg_sample_plan; anything else (11 included) -> -1.  Callable without a GPU. */
#define FSG_SIZEOF_SAMPLE_PLAN 0
#define FSG_SIZEOF_TAP 6
#define FSG_SIZEOF_DEFORM 7
#define FSG_SIZEOF_EPILOGUE 8
#define FSG_SIZEOF_KEYED_CONFIG 9
#define FSG_SIZEOF_KEYED_DRAWS 10
#define FSG_SIZEOF_SAMPLE_IMAGE 12
#define FSG_SIZEOF_KEYED_OVERRIDES 13
int64_t fsg_sample_plan_layout(int which);
/* B samples with one call: plan b runs on streams[b % nstreams] (hipStream_t handles).  The caller orders those streams
 * behind the upload of every plan's parameters and waits for them afterwards; per sample the work is exactly
 * fsg_sample_run's (reference: B consecutive FetalSynthGen.sample calls, generator/model.py:231-276; the reference's
 * DataLoader collates B such samples, data/datasets.py:310-325, docs/datasets.md:4-6). */
/* The plan from two flat arrays (one FFI call instead of a field-by-field fill): iv[FSG_PLAN_I_*] integers and pointers as
 * int64, fv[FSG_PLAN_F_*] doubles that hold float32 values exactly, taps = 3 x FSG_PLAN_TAPS_STRIDE floats (row a = the
 * blur taps of axis a, FSG_PLAN_I_BLUR_NTAPS + a of them).  fsg_sample_pack_run = pack + fsg_sample_run. */
enum {
  FSG_PLAN_I_SHAPE = 0, FSG_PLAN_I_LABEL_PARTS = 3, FSG_PLAN_I_MUS = 7, FSG_PLAN_I_SIGMAS = 8, FSG_PLAN_I_NTAB = 9,
  FSG_PLAN_I_GMM_NOISE = 10, FSG_PLAN_I_GMM_SEED = 11, FSG_PLAN_I_GMM_STREAM = 12, FSG_PLAN_I_DEFORM_ACTIVE = 13,
  FSG_PLAN_I_FLIP = 14, FSG_PLAN_I_FIELD_DIMS = 15, FSG_PLAN_I_FIELD = 18, FSG_PLAN_I_FIELD_TABS = 19, FSG_PLAN_I_SEG_IN = 22,
  FSG_PLAN_I_SEG_OUT = 23, FSG_PLAN_I_SEG_IN_U8 = 24, FSG_PLAN_I_BIAS_DIMS = 25, FSG_PLAN_I_BIAS = 28, FSG_PLAN_I_BIAS_TABS = 29,
  FSG_PLAN_I_RESAMPLE_ACTIVE = 32, FSG_PLAN_I_LOW_SHAPE = 33, FSG_PLAN_I_RS_TABS = 36, FSG_PLAN_I_BACK_TABS = 39,
  FSG_PLAN_I_BLUR_NTAPS = 42, FSG_PLAN_I_NOISE_MODE = 45, FSG_PLAN_I_NOISE = 46, FSG_PLAN_I_NOISE_SEED = 47,
  FSG_PLAN_I_NOISE_STREAM = 48, FSG_PLAN_I_SCALE01 = 49, FSG_PLAN_I_WS0 = 50, FSG_PLAN_I_WS1 = 51, FSG_PLAN_I_WS_LOW = 52,
  FSG_PLAN_I_WS_ROWS = 53, FSG_PLAN_I_ROW_STRIDE = 54, FSG_PLAN_I_MM8 = 55, FSG_PLAN_I_MM8_PRESET = 56, FSG_PLAN_I_OUT = 57,
  FSG_PLAN_I_EV_BEGIN = 58, FSG_PLAN_I_EV_END = 59, FSG_PLAN_I_MM_SLOTS = 60, FSG_PLAN_I_MM_NSLOTS = 61, FSG_PLAN_I_ARENA_HOST = 62,
  FSG_PLAN_I_ARENA_DEV = 63, FSG_PLAN_I_ARENA_BYTES = 64, FSG_PLAN_I_OVERLAP = 65, FSG_PLAN_I_WS_SEQ = 66, FSG_PLAN_I_SEG_OUT_U8 = 67,
  FSG_PLAN_I_TRACE_EVENTS = 68, FSG_PLAN_I_TRACE_IDS = 69, FSG_PLAN_I_TRACE_CAP = 70, FSG_PLAN_I_COUNT = 71
};
enum { FSG_PLAN_F_A = 0, FSG_PLAN_F_CENTRE = 9, FSG_PLAN_F_C2 = 12, FSG_PLAN_F_GAMMA = 15, FSG_PLAN_F_NOISE_STD = 16, FSG_PLAN_F_COUNT = 17 };
#define FSG_PLAN_TAPS_STRIDE 132
int fsg_sample_plan_pack(fsg_sample_plan* plan, const int64_t* iv, int niv, const double* fv, int nfv, const float* taps);
int fsg_sample_pack_run(const int64_t* iv, int niv, const double* fv, int nfv, const float* taps, void* stream);
int fsg_sample_run_batch(const fsg_sample_plan* plans, int nplans, void* const* streams, int nstreams);

/* ---- K6 + K7 (+ K8) fused per axis (csrc/fsg_blur_rs.hip) -----------------------------------------------------------
 * RandResample.__call__ (generator/augmentation/synthseg.py:50-107) = gaussian_blur_3d (utils/generation.py:84-110) then the
 * axis-aligned trilinear down-sampling (synthseg.py:84-104 -> utils/generation.py:227-278), RandNoise after it (synthseg.py:
 * 230-233).  Blur and resampling are separable linear operators, so per axis they combine into one FIR with position-dependent
 * coefficients (w_lo k[.] + w_hi k[. - 1]) evaluated for the m low-res outputs only; the blurred full-resolution volume is
 * never formed.  Two launches: x (reads N, writes N m0/n0), then y + z + noise (reads N m0/n0, writes M).  Results equal
 * the unfused sequence (fsg_blur_axis_* x3, fsg_resample_noise_f32) up to float32 rounding of a re-ordered linear map --
 * within the blur's own tolerance (atol 1e-3 on the 0..255 scale).  Zero-padded un-renormalised borders, noise and the clamp
 * at 0 after, as in the reference.  Tables: down-sampling, m < n on every axis (else FSG_E_ALIGN), every output inside
 * (lo >= 0), lo strictly increasing, hi = lo or lo + 1 (not checked here: kernels.DeviceTables records it); an output
 * outside (0, n-1] -- output 0 when m == n -- is never written.
 * taps: odd counts 3..17 (radius 1..8) on all three axes; n2 % 4 == 0, n2 <= 512, the y,z launch's LDS <= 64000 bytes;
 * otherwise FSG_E_ALIGN (callers then use the unfused entry points).  x launch: FSG_E_TOOBIG unless
 * (16 ceil(n0 / 16) + R_x + 1) * n1 * n2 * 4 <= 2^32 (its 32-bit row offsets must not wrap).
 * fsg_blur_resample_supported: 1 when both launches accept the configuration (no GPU call). */
int fsg_blur_resample_supported(int n0, int n1, int n2, int m0, int m1, int m2, int ntaps_x, int ntaps_y, int ntaps_z);
int fsg_blur_resample_x_f32(const float* src, int n0, int n1, int n2, const fsg_tap* tx, int m0, const float* taps_host,
                            int ntaps, float* dst, void* stream);
int fsg_blur_resample_yz_noise_f32(const float* src, int m0, int n1, int n2, const fsg_tap* ty, const fsg_tap* tz, int m1,
                                   int m2, const float* taps_y_host, int ntaps_y, const float* taps_z_host, int ntaps_z,
                                   int noise_mode, const float* noise, uint64_t seed, uint64_t stream_id, float noise_std,
                                   float* dst, void* stream);

/* ---- keyed mode: every per-sample draw from a counter-based generator keyed (base_seed, sample index) --------------------
 * The reference draws a sample's ~30 scalars and its small tensors from numpy's / torch's GLOBAL generators, one Python call
 * each, in an order that is part of its behaviour (rand_gmm.py:82-85,:120-148, affine_nonrigid.py:140-145,
 * :248-263,:284,:303-318, synthseg.py:263-265,:157-176,:63-78,:218-232).  `rng="reference"` / `"device"` replay that tape on
 * the host (~100 interpreter round trips per sample).  Keyed mode keeps the DISTRIBUTIONS and the arithmetic that turns draws
 * into parameters, but takes every uniform / normal from Philox4x32-10 under the sample's 64-bit key (a fixed counter per
 * draw, so gates do not shift later draws): the scalars are drawn in C inside fsg_keyed_sample_run, the small tensors (GMM
 * tables, coarse displacement grid, bias grid) by a one-launch device kernel straight into the sample's parameter block, the
 * two large fields in the kernels that consume them (as in "device" mode).  The host hands over pointers and the key.
 * A sample depends on its key only -- not on the process, the GPU count or what ran before ("(base_seed,
 * sample_index) keyed RNG").  Parity: fsg_keyed_draws exports what was drawn; tests feed it to the oracle.
 *
 * Overrides (fsg_keyed_overrides: the reference's `genparams`, generator/model.py:231-276).  Because every draw sits at a fixed
 * counter, a caller can replace the VALUE of single draws and leave the rest of the key's sample alone:
 *   - no draw moves: an override replaces one value; only what is derived from it changes (A from rotations / shears /
 *     scalings, field_dims from field_dims | nonlin_scale, bias_dims from bf_scale, per-axis stds / low_shape / blur_ntaps from
 *     the 3-vector spacing, noise_std32 from noise_std), by the same code that derives it from drawn values; c2 and u_std always
 *     come from the key;
 *   - gates are forced where the reference's plan() methods force them: deformation by FSG_KO_FORCE_DEFORM or any deformation
 *     field, bias by FSG_KO_FORCE_BIAS or bf_scale / bf_std, gamma / resampling / noise by their value; the members of a forced
 *     stage that are not given take the key's own slot values (they exist whether or not the key's gate fired);
 *   - mus_dev / sigmas_dev (ntab floats each, DEVICE) replace the respective table draw of the draw kernel, each on its own;
 *     with tied classes the tie step still runs on top of given means, with the key's normals (rand_gmm.py:139-145);
 *   - what cannot be honoured is refused: FSG_E_BADARG for a non-finite value, gamma <= 0, spacing <= 0, a low-res or grid
 *     size < 1, a sub-cluster count outside [min_subclusters, max_subclusters], ntab != nlabels or a null table; FSG_E_TOOBIG
 *     for a low-res or grid size above the table cap (1024) or a parameter block of 2 GiB or more.
 * With no override every byte of the draws and of the block is what it is without the argument.
 */
typedef struct fsg_keyed_config {
  int32_t shape[3];
  int32_t size[3];                 /* SpatialDeformation(size=...)                                   */
  double resolution[3];
  int32_t min_subclusters, max_subclusters, meta_labels;   /* ImageFromSeeds; meta_labels <= 4       */
  int32_t nlabels;                 /* max(seed_labels) + 1 <= 256                                    */
  int32_t n_seed_labels;           /* len(seed_labels) == len(generation_classes) <= 256             */
  int32_t tie_classes;             /* generation_classes != seed_labels (rand_gmm.py:139-145)        */
  uint8_t seed_labels[256];
  uint8_t generation_classes[256];
  double deform_prob, flip_prb, max_rotation, max_shear, max_scaling;
  int32_t nonlinear;
  double nonlin_scale_min, nonlin_scale_max, nonlin_std_max;
  double gamma_prob, gamma_std;
  double bias_prob, bf_scale_min, bf_scale_max, bf_std_min, bf_std_max;
  double resample_prob, min_resolution, max_resolution;
  double noise_prob, noise_std_min, noise_std_max;
} fsg_keyed_config;

typedef struct fsg_keyed_draws {
  uint64_t key;
  int32_t subclusters[4];          /* mlabel m+1 -> number of sub-clusters                           */
  int32_t ntab;
  int32_t deform_active, flip;
  double rotations[3], shears[3], scalings[3];
  float A[9];
  double c2[3];
  int32_t nonlinear;
  double nonlin_scale, nonlin_std;
  int32_t field_dims[3];
  int32_t gamma_active;
  double gamma;
  int32_t bias_active;
  double bf_scale, bf_std;
  int32_t bias_dims[3];
  int32_t resample_active;
  double spacing, u_std, stds[3];
  int32_t low_shape[3];
  int32_t blur_ntaps[3];
  int32_t noise_active;
  double noise_std;
  float noise_std32;
  /* Prior mode (FSG_KEYED_I_PRIOR_IN): every draw keeps its fixed counter, so the deformation, gamma, bias, resampling and noise
   * fields above and below are those of the same key in seed mode; subclusters / ntab (and mus / sigmas in the block) are
   * UNSPECIFIED there -- nothing reads them. */
  /* byte offsets into the sample's device parameter block of what the draw kernel writes there */
  int32_t off_mm8, off_slots, off_mus, off_sigmas, off_bias, off_field, block_bytes;
  int32_t rode; /* fsg_keyed_sample_run: 1 when the draw job of the NEXT sample went out with this one (look-ahead) */
  double spacing3[3];              /* per-axis spacing (an override may give three); spacing == spacing3[0] */
  uint32_t overridden;             /* FSG_KO_* of what the caller fixed (0: every value is the key's)       */
  uint64_t mus_in, sigmas_in;      /* DEVICE addresses of given GMM tables (0: drawn), read by the draw kernel */
} fsg_keyed_draws;

/* Presence bits of fsg_keyed_overrides::mask.  FORCE_DEFORM / FORCE_BIAS carry no value: the stage's gate alone. */
#define FSG_KO_SUBCLUSTERS 1
#define FSG_KO_FLIP 2
#define FSG_KO_ROTATIONS 4
#define FSG_KO_SHEARS 8
#define FSG_KO_SCALINGS 16
#define FSG_KO_NONLIN_SCALE 32
#define FSG_KO_NONLIN_STD 64
#define FSG_KO_FIELD_DIMS 128
#define FSG_KO_GAMMA 256
#define FSG_KO_BF_SCALE 512
#define FSG_KO_BF_STD 1024
#define FSG_KO_SPACING 2048
#define FSG_KO_NOISE_STD 4096
#define FSG_KO_MUS 8192
#define FSG_KO_SIGMAS 16384
#define FSG_KO_FORCE_DEFORM 32768
#define FSG_KO_FORCE_BIAS 65536
typedef struct fsg_keyed_overrides {
  uint32_t mask;                   /* which of the fields below are given                           */
  int32_t subclusters[4];          /* mlabel m+1 -> number of sub-clusters (the first meta_labels)   */
  int32_t flip;
  double rotations[3], shears[3], scalings[3];
  double nonlin_scale, nonlin_std;
  int32_t field_dims[3];           /* size_F_small: wins over nonlin_scale                           */
  double gamma;
  double bf_scale, bf_std;
  double spacing[3];
  double noise_std;
  int32_t ntab;                    /* entries of each given table: must equal nlabels                */
  uint64_t mus_dev, sigmas_dev;    /* DEVICE float32 tables (FSG_KO_MUS / FSG_KO_SIGMAS)             */
} fsg_keyed_overrides;

enum { FSG_KT_RESAMPLE = 0, FSG_KT_BACK = 1, FSG_KT_FIELD = 2, FSG_KT_BIAS = 3 };
/* Host-only object (no HIP call, usable without a GPU).  *ctx receives the handle. */
int fsg_keyed_create(const fsg_keyed_config* cfg, void** ctx);
int fsg_keyed_destroy(void* ctx);
/* Registers the DEVICE tap table of (kind, axis, n): FSG_KT_RESAMPLE / FSG_KT_BACK: n = low-res size along `axis`;
 * FSG_KT_FIELD / FSG_KT_BIAS: n = coarse grid size along `axis`.  The tables are the ones the other modes use (built by the
 * host mirror with the reference's own torch calls, utils/generation.py:315-363, synthseg.py:84-102), so sampling positions
 * stay bit-identical.  A sample that needs an unregistered table fails with FSG_E_NOTABLE. */
int fsg_keyed_set_table(void* ctx, int kind, int axis, int n, const fsg_tap* table_dev);
/* Bytes of the per-sample device parameter block for the largest grids this configuration can draw. */
int64_t fsg_keyed_block_bytes(void* ctx);
/* Host draws of the sample `key` (no device work): what fsg_keyed_sample_run will use. */
int fsg_keyed_draw(void* ctx, uint64_t key, fsg_keyed_draws* out);
/* The same with overrides (NULL or mask 0: exactly fsg_keyed_draw).  out->block_bytes may exceed fsg_keyed_block_bytes: the
 * caller then allocates that much (FSG_KEYED_I_BLOCK_BYTES). */
int fsg_keyed_draw_with(void* ctx, uint64_t key, const fsg_keyed_overrides* overrides, fsg_keyed_draws* out);
/* One sample: draws + the draw kernel + fsg_sample_run's launch sequence.  iv (int64): FSG_KEYED_I_*.
 * bank: FSG_KEYED_I_BANK + 4 * (n_sub - min_subclusters) + (mlabel - 1) -> uint8 seed volume of (n_sub, mlabel).
 * draws_out may be NULL. */
enum {
  FSG_KEYED_I_KEY = 0, FSG_KEYED_I_OUT = 1, FSG_KEYED_I_SEG_OUT = 2, FSG_KEYED_I_SEG_OUT_U8 = 3, FSG_KEYED_I_SEG_IN = 4,
  FSG_KEYED_I_SEG_IN_U8 = 5, FSG_KEYED_I_BLOCK = 6, FSG_KEYED_I_WS0 = 7, FSG_KEYED_I_WS1 = 8, FSG_KEYED_I_WS_LOW = 9,
  FSG_KEYED_I_WS_ROWS = 10, FSG_KEYED_I_ROW_STRIDE = 11, FSG_KEYED_I_SCALE01 = 12, FSG_KEYED_I_TRACE_EVENTS = 13,
  FSG_KEYED_I_TRACE_IDS = 14, FSG_KEYED_I_TRACE_CAP = 15, FSG_KEYED_I_BANK = 16, FSG_KEYED_I_EV_BLUR_BEGIN = 16 + 64,
  FSG_KEYED_I_EV_BLUR_END = 16 + 65,
  /* optional code volume of the subject (0 = none): uint16 codes, uint8 tuples [ntuples][stride] whose byte
   * 4 * (n_sub - min_subclusters) + (mlabel - 1) is the value of seed volume (n_sub, mlabel) and whose byte stride - 1 is 0 */
  FSG_KEYED_I_CODES = 16 + 66, FSG_KEYED_I_CODE_TUPLES = 16 + 67, FSG_KEYED_I_CODE_NTUPLES = 16 + 68, FSG_KEYED_I_CODE_STRIDE = 16 + 69,
  /* look-ahead (optional).  FLAGS bit 0 (FSG_KEYED_FLAG_BLOCK_FILLED): the block of THIS sample is already filled (the previous
   * call carried its draw job); bit 2 (FSG_KEYED_FLAG_NEXT_NAMED): NEXT_KEY / NEXT_BLOCK name the sample the caller will run next
   * on this stream -- its draw job then rides in this sample's head launch (fsg_keyed_draws::rode says whether it did: not
   * when the deformation gate is off, nor when the job is too large to be carried).  A caller that then runs something else simply does not set bit 0.  (r03: the next sample's GMM draw beside the zoom-back launches was built
   * and measured too -- 224 -> 230-244 us per step, the two jobs slow each other down -- and removed.) */
  FSG_KEYED_I_FLAGS = 16 + 70, FSG_KEYED_I_NEXT_KEY = 16 + 71, FSG_KEYED_I_NEXT_BLOCK = 16 + 72,
  /* real-image samples (optional, 0 = none): fsg_sample_image::image_in / image_out / prior_in.  With PRIOR_IN the BANK and CODES
   * slots are not read (a subject without seeds); with a bank and IMAGE_IN the synthetic channel is that of the same key without an image.
   * The look-ahead does not care which kind the next sample is: its draw job is the same. */
  FSG_KEYED_I_IMAGE_IN = 16 + 73, FSG_KEYED_I_IMAGE_OUT = 16 + 74, FSG_KEYED_I_PRIOR_IN = 16 + 75,
  FSG_KEYED_I_COUNT = 16 + 76,
  /* overrides: two slots BEHIND the count every caller passes, read only when niv >= FSG_KEYED_I_COUNT_OV (a caller of the
   * shorter array gets a sample without overrides).  OVERRIDES: HOST address of a fsg_keyed_overrides for THIS sample (0 = none;
   * the look-ahead's next sample never has any).  BLOCK_BYTES: capacity of the block at FSG_KEYED_I_BLOCK
   * (0 = fsg_keyed_block_bytes): overridden grids may be larger than the configuration's maximum. */
  FSG_KEYED_I_OVERRIDES = 16 + 76, FSG_KEYED_I_BLOCK_BYTES = 16 + 77, FSG_KEYED_I_COUNT_OV = 16 + 78
};
#define FSG_KEYED_FLAG_BLOCK_FILLED 1
#define FSG_KEYED_FLAG_NEXT_NAMED 4
int fsg_keyed_sample_run(void* ctx, const int64_t* iv, int niv, fsg_keyed_draws* draws_out, void* stream);
/* The draw kernel alone (tests): fills the parameter block of `draws` at block_dev (at least draws->block_bytes; given
 * tables are read from draws->mus_in / sigmas_in, which may be the block's own table addresses). */
int fsg_keyed_fill_block(void* ctx, const fsg_keyed_draws* draws, void* block_dev, void* stream);

/* Retired with fsg_sample_plan::overlap: the library owns no streams or events any more.  Kept for the ABI; returns 0. */
int fsg_pipeline_teardown(void);
/* float32 -> float16 (round to nearest even) copy of a volume: the optional half-precision image of the output side. */
int fsg_cast_f32_to_f16(const float* x, size_t n, void* out_f16, void* stream);

/* hipEvent helpers for ctypes callers (timing on the launch stream). elapsed_ms synchronises on `end`. */
void* fsg_event_create(void);
int fsg_event_record(void* event, void* stream);
int fsg_event_destroy(void* event);
int fsg_event_elapsed_ms(void* begin, void* end, float* ms);

/* ---------------------------------------------------------------------------------------------------------------------
 * Seed generation (fsg_seedgen.hip): what scripts/generate_seeds.py of the reference does offline with sklearn.
 *
 * Meta-label fusion + stable compaction.  Exactly one of seg_u8 / seg_f32 is given.  NaN in image or label counts as 0;
 * a label equal to clear_label (-1 = none) is set to 0 first; meta = table256[label] (values 0..4); label 0 with a non-zero
 * image value -> 4.  Outputs: the uint8 meta volume, counts4[m-1] = voxels of meta-label m, and packed_x / packed_idx
 * (n entries each): the intensities and voxel indices of meta-label 1, then 2, 3, 4, each in voxel order -- the order
 * is a function of the inputs alone.  work: fsg_seed_meta_work_bytes(n) bytes.  Three launches, no host sync. */
size_t fsg_seed_meta_work_bytes(size_t n);
int fsg_seed_meta_pack(const uint8_t* seg_u8, const float* seg_f32, const float* image, size_t n, const uint8_t* table256,
                       int clear_label, uint8_t* meta, uint32_t* counts4, float* packed_x, int32_t* packed_idx, void* work,
                       void* stream);

/* Batched 1-D Gaussian-mixture EM.  jobs_host: HOST table, 8 int64 per job:
 *   [0] offset of the job's samples in x   [1] n samples   [2] k components (1..16)
 *   [3] first workgroup of the job   [4] its workgroup count = ceil(n / tile)   (consecutive over the table; tile from the
 *       call below)   [5] max_iter (>= 1)   [6] 0 = params holds initial weights/means/variances, 1 = params holds initial
 *       means only (one-hot responsibilities of the nearest mean, then an M-step), 2 = no fit (params are final: assignment only)   [7] 0
 * tol_host: HOST, one double per job (>= 0; 0 = run max_iter iterations).  params: DEVICE double [njobs][3][16] (weights,
 * means, variances; in: initial, out: fitted).  lower_bound: DEVICE double [njobs].  status: DEVICE int32 [njobs][4] =
 * n_iter, converged, done, 0.  work: DEVICE, 16-byte aligned, at least the work-bytes call says for (njobs, total workgroups).
 * The two host tables are copied to the device on `stream` (they must stay valid until the stream has passed the copies); then
 * two launches per iteration up to the largest max_iter, no host synchronisation, workgroups of finished jobs return at once.
 * Sums are float64 and reduced in a fixed order: results are bitwise reproducible and independent of the job order.
 * FSG_E_BADARG: null pointer, k < 1 or k > 16, n == 0 with k > 1, max_iter < 1, a job outside x, inconsistent workgroup ranges. */
int fsg_em1d_tile(void);
size_t fsg_em1d_work_bytes(int njobs, int64_t nblocks);
int fsg_em1d_fit(const float* x, size_t nx, int njobs, const int64_t* jobs_host, const double* tol_host, double* params,
                 double* lower_bound, int32_t* status, void* work, size_t work_bytes, void* stream);

/* Assignment + scatter for nwin jobs of the table the fit ran on (same work buffer).  wins_host: HOST, 4 int64 per entry: job
 * index, DEVICE pointer of a zero-filled uint8 volume, base value, first workgroup (consecutive, job's workgroup count each).
 * out[packed_idx[i]] = base + rank of the component with the largest weighted log-density (ties -> lowest component), where
 * rank orders the components by ascending mean. */
int fsg_seed_assign(const float* x, size_t nx, const int32_t* packed_idx, int njobs, const int64_t* jobs_host, int nwin,
                    const int64_t* wins_host, const double* params, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Regridding of real volumes (fsg_regrid.hip): what scripts/resample.py and the transforms of data/datasets.py:106-186
 * (FetalTestDataset; transforms/inference.yaml) do on the host with monai -- spacing change, RAS reorientation, foreground
 * crop, centre crop and zero pad, and their inverses -- as ONE resample through a composed voxel-to-voxel affine.
 *
 * For every output voxel (i,j,k) of (d0,d1,d2): p = M (i,j,k,1), M_host = 12 HOST floats, row-major 3x4, output index ->
 * source voxel coordinate, evaluated in float32 as (m0 i + m1 j) + m2 k + m3 with separate multiplies and adds from the
 * voxel's index (never accumulated): exact whenever every product and partial sum is representable, within 2^-13 of the
 * float64 value for extents <= 512.  box_host = 6 HOST int32 lo0,hi0,lo1,hi1,lo2,hi2: the inclusive source index box that
 * counts as inside.  A voxel is inside iff lo_a - 0.5 <= p_a <= hi_a + 0.5 on all axes; outside voxels receive fill /
 * fill_label (converted to the label dtype).  Inside, p is clamped to [lo_a, hi_a] (border replication within the box) and
 *   out       = trilinear(src): f = floor(p), upper neighbour clamped to hi_a, weights 1-w and w, z then y then x,
 *               separate multiplies and adds; nan_is_zero != 0: a NaN source voxel reads as 0;
 *   out_label = src_label at rint(p) (ties to even), copied; label_dtype = FSG_LABEL_* of BOTH label volumes.
 * Either pair (src, out) / (src_label, out_label) may be NULL, not both.  One launch, no coordinate volumes.
 * FSG_E_BADARG: a pair given by half, in place, a non-positive extent, a box that is empty or leaves the source, a
 * non-finite entry of M, an unknown label_dtype; FSG_E_TOOBIG: an extent above 1024. */
#define FSG_LABEL_U8 0
#define FSG_LABEL_I16 1
#define FSG_LABEL_F32 2
int fsg_affine_resample(const float* src, const void* src_label, int label_dtype, int s0, int s1, int s2, const float* M_host,
                        const int32_t* box_host, int d0, int d1, int d2, float* out, void* out_label, float fill,
                        float fill_label, int nan_is_zero, void* stream);
/* box6_dev (DEVICE, 6 int32) = lo0,hi0,lo1,hi1,lo2,hi2 of the voxels with v > thr (NaN compares false); an empty set gives
 * lo = n, hi = -1 on every axis.  Per-workgroup reduction, then integer atomicMin / atomicMax: independent of the order.
 * Two launches (the reset of the six words, the reduction).  What CropForeground's select_fn = (x > 0) computes. */
int fsg_bbox_gt_f32(const float* v, int n0, int n1, int n2, float thr, int32_t* box6_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FSG_HIP_H */
