/*
 * mifwt.h — C ABI of libmifwt.so, the MI355X (gfx950) fast-wavelet-transform engine.
 *
 * Drop-in seam.  The reference (v0lta/PyTorch-Wavelet-Toolbox, "ptwt") is pure Python and has no FFI;
 * this ABI sits exactly where the reference hands one decomposition / reconstruction level to ATen:
 *
 *   analysis  level : F.pad (or _pad_symmetric) + F.conv{1,2,3}d(stride=2) + torch.split
 *       src/ptwt/conv_transform.py:135-139     (1-D:  _fwt_pad :33-66,  conv1d :137)
 *       src/ptwt/conv_transform_2.py:142-149   (2-D:  _fwt_pad2 :34-71, conv2d :144)
 *       src/ptwt/conv_transform_3.py:121-141   (3-D:  _fwt_pad3 :34-73, conv3d :127)
 *       src/ptwt/separable_conv_transform.py:38-72 (separable: the same level, axis by axis)
 *   synthesis level : torch.stack + F.conv_transpose{1,2,3}d(stride=2) + crop
 *       src/ptwt/conv_transform.py:184-199, conv_transform_2.py:222-249, conv_transform_3.py:205-249,
 *       src/ptwt/separable_conv_transform.py:75-111
 *
 * One call = one level for the whole (folded) batch = ONE fused kernel on the fast paths: the boundary
 * extension is an index map inside the kernel (no padded tensor in HBM), the 2^ndim sub-bands are written
 * straight to their final planes (no split/stack copies) and only the cropped interior of a synthesis
 * level is computed.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers owned by the caller (torch's caching allocator); filter taps
 *     are HOST pointers (double, PyWavelets order, NOT flipped — the library applies the flip the
 *     reference does at src/ptwt/_util.py:863-865).  Taps are copied into the kernel arguments, so there
 *     is no device-side filter state and calls are re-entrant.
 *   - Nothing here allocates, frees or synchronises.  Work is enqueued on `stream`
 *     (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) of the current HIP device.
 *   - Strides are in ELEMENTS.  Index 0 of every stride array is the folded batch, then the transformed
 *     axes outermost first.  The innermost transformed axis need not be contiguous (arbitrary strides are
 *     accepted; unit innermost stride selects the fused fast kernels).
 *   - Sub-band order: band index s in [0, 2^ndim); bit (ndim-1-a) of s set <=> axis a is HIGH-pass
 *     ("aa","ad","da","dd" / "aaa","aad",...,"ddd": character i of the key <-> transformed axis i,
 *     as in src/ptwt/_util.py:926-934).  Band 0 is the approximation; details[s-1] is band s.
 *     (ptwt's 2-D tuple is (H,V,D) = ('da','ad','dd') = details[1], details[0], details[2].)
 *   - Return value: MIFWT_OK or a negative error code; never throws.
 */
#ifndef MIFWT_H
#define MIFWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIFWT_ABI_VERSION 3
#define MIFWT_MAX_NDIM 3
#define MIFWT_MAX_FILT 128 /* longest PyWavelets discrete filter is coif17 = 102 taps */

enum mifwt_dtype {
  MIFWT_F32 = 0,
  MIFWT_F64 = 1,
  MIFWT_F16 = 2, /* f16 storage, f32 arithmetic */
  MIFWT_BF16 = 3 /* bf16 storage, f32 arithmetic */
};
/* The two 16-bit STORAGE types go together: every entry point that takes MIFWT_F16 takes MIFWT_BF16, runs it on the same kernel id (a
 * bf16 instantiation of that kernel) and rounds where the f16 form rounds — mifwt_dwt_fwd / _inv and their adjoints (kernel ids 0, 3 - 8,
 * 11, 23), mifwt_kernel_id, mifwt_workspace_bytes, mifwt_swt_fwd / mifwt_swt_inv.  Every entry point that answers MIFWT_ERR_UNSUPPORTED
 * (or 0 from a *_supported query) for MIFWT_F16 answers the same for MIFWT_BF16, never MIFWT_ERR_BADARG: the multi-level launches,
 * mifwt_dwt1_*_outer, mifwt_swt2_* / mifwt_swt3_*, mifwt_tap_correlate*, mifwt_per_*, mifwt_ext_*, mifwt_bwt_*, mifwt_bwt3_* and
 * mifwt_bwt_tree_*.  The device-tap entry points (_dtaps) take both types where their kernels do (ids 0, 3, 4, 7, 8).  Added within ABI
 * version 3: a new enumerator changes no existing call. */

/* Boundary rules of ptwt.constants.BoundaryMode (src/ptwt/constants.py:85-108, _util.py:36-44). */
enum mifwt_mode {
  MIFWT_MODE_ZERO = 0,      /* ... 0  0 | x1 x2 ... xn | 0  0 ...        (torch "constant")  */
  MIFWT_MODE_CONSTANT = 1,  /* ... x1 x1 | x1 x2 ... xn | xn xn ...      (torch "replicate") */
  MIFWT_MODE_REFLECT = 2,   /* ... x3 x2 | x1 x2 ... xn | xn-1 xn-2 ...  (torch "reflect")   */
  MIFWT_MODE_PERIODIC = 3,  /* ... xn-1 xn | x1 x2 ... xn | x1 x2 ...    (torch "circular")  */
  MIFWT_MODE_SYMMETRIC = 4  /* ... x2 x1 | x1 x2 ... xn | xn xn-1 ...    (_pad_symmetric)    */
};

enum mifwt_status {
  MIFWT_OK = 0,
  MIFWT_ERR_BADARG = -1,      /* null pointer, ndim/dtype/mode/filt_len out of range, extents inconsistent */
  MIFWT_ERR_UNSUPPORTED = -2, /* valid request this build has no kernel for */
  MIFWT_ERR_WORKSPACE = -3,   /* workspace smaller than mifwt_workspace_bytes() */
  MIFWT_ERR_LAUNCH = -4       /* hipLaunchKernel reported an error (see hipGetLastError) */
};

/* One decomposition / reconstruction level of an ndim-dimensional transform over a folded batch. */
typedef struct mifwt_level_desc {
  int32_t ndim;     /* 1..3 transformed axes */
  int32_t dtype;    /* enum mifwt_dtype */
  int32_t mode;     /* enum mifwt_mode (analysis only; synthesis ignores it) */
  int32_t filt_len; /* L, 2..MIFWT_MAX_FILT */
  int64_t batch;    /* folded leading dims (src/ptwt/_util.py:271-286) */
  /* signal side: analysis input / synthesis output.  Synthesis output extent per axis must be
   * 2*M - L + 2 - t with t in {0,1}: t = 1 is the reference's extra end-crop
   * (src/ptwt/_util.py:231-244); only these samples are computed. */
  int64_t sig_extent[MIFWT_MAX_NDIM];
  int64_t sig_stride[1 + MIFWT_MAX_NDIM];
  /* coefficient side: every sub-band has extent M = floor((N + L - 1) / 2) per axis
   * (= the conv output length of src/ptwt/_util.py:204-217; passed, not recomputed). */
  int64_t coef_extent[MIFWT_MAX_NDIM];
  int64_t approx_stride[1 + MIFWT_MAX_NDIM]; /* band 0 */
  int64_t detail_stride[1 + MIFWT_MAX_NDIM]; /* bands 1..2^ndim-1 share one stride set */
} mifwt_level_desc;

/* Replaces: F.pad/_pad_symmetric + F.conv{1,2,3}d(stride=2) + split (citations above).
 *   x        analysis input                        [batch, N_0.., N_{ndim-1}] via sig_stride
 *   approx   band 0 output                         [batch, M_0..]             via approx_stride
 *   details  HOST array of 2^ndim-1 device ptrs    [batch, M_0..] each        via detail_stride
 *   dec_lo/dec_hi  HOST taps, PyWavelets order (wavelet.dec_lo / dec_hi), L doubles each
 *   workspace      device scratch of >= mifwt_workspace_bytes(desc, 0) bytes (may be NULL if that is 0) */
int mifwt_dwt_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details,
                  const double* dec_lo, const double* dec_hi, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Replaces: torch.stack + F.conv_transpose{1,2,3}d(stride=2) + crop (citations above).
 *   approx / details  inputs laid out as above;  y  output [batch, sig_extent..] via sig_stride
 *   rec_lo/rec_hi     HOST taps, PyWavelets order (wavelet.rec_lo / rec_hi) */
int mifwt_dwt_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y,
                  const double* rec_lo, const double* rec_hi, void* workspace, size_t workspace_bytes,
                  void* stream);

/* DEVICE-RESIDENT TAPS (rounds 5 / 6).  The entry points above take the filter as HOST doubles (the kernels receive it in their launch
 * arguments); a learnable filter bank that lives on the GPU (the reference keeps its taps as tensors with autograd,
 * src/ptwt/_util.py:115-132; examples/network_compression/wavelet_linear.py:118,150) would have to be copied to the host — a stream
 * synchronisation — on every call.  These four take DEVICE pointers to L doubles each; the kernels read the taps themselves: no copy,
 * no synchronisation, capturable into a HIP graph.  Which kernel serves a call: mifwt_kernel_id_dtaps(desc, direction) — the fused 2-D
 * kernels where they read device taps (round 6: LDS tiles, ids 7 / 8: every dtype and filter length they serve; one level through the
 * streaming kernels, ids 16 / 22; the border kernels of the analysis adjoint; the streaming axis passes, ids 3 / 4: what a learnable-wavelet training step on image-sized
 * planes runs on, src/ptwt/_util.py:115-132), the generic per-axis passes (id 0: every dtype, mode, stride set and filter length)
 * everywhere else.  A kernel reads the L doubles once, when it starts, into the registers its by-value taps would occupy (same
 * conversion, same packing): results are bit-identical to the host-tap entry points on the same kernel.
 * Workspace: mifwt_workspace_bytes_dtaps(desc, direction), direction as for mifwt_workspace_bytes (0 .. 3). */
int mifwt_kernel_id_dtaps(const mifwt_level_desc* desc, int direction);
size_t mifwt_workspace_bytes_dtaps(const mifwt_level_desc* desc, int direction);
int mifwt_dwt_fwd_dtaps(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* d_dec_lo,
                        const double* d_dec_hi, void* workspace, size_t workspace_bytes, void* stream);
int mifwt_dwt_inv_dtaps(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* d_rec_lo,
                        const double* d_rec_hi, void* workspace, size_t workspace_bytes, void* stream);
int mifwt_dwt_fwd_adjoint_dtaps(const mifwt_level_desc* desc, const void* g_approx, const void* const* g_details, void* g_x,
                                const double* d_dec_lo, const double* d_dec_hi, void* workspace, size_t workspace_bytes, void* stream);
int mifwt_dwt_inv_adjoint_dtaps(const mifwt_level_desc* desc, const void* g_y, void* g_approx, void* const* g_details,
                                const double* d_rec_lo, const double* d_rec_hi, void* workspace, size_t workspace_bytes, void* stream);

/* Round 6, for the tap gradients of 2-D levels with every operand in its natural layout (no transposed copies):
 * mifwt_dwt1_fwd_outer — one 1-D analysis level along the MIDDLE axis of [batch, n, inner] arrays (inner contiguous; element strides):
 *   lo_out / hi_out [batch, floor((n + L - 1) / 2), inner]; taps as HOST doubles (dec_lo / dec_hi) or, when d_dec_lo / d_dec_hi are non-null,
 *   DEVICE doubles (the host pointers are then ignored).  f32 / f64, the filter lengths of the streaming axis kernels (even L <= 20, 24, 32).
 * mifwt_dwt1_inv_outer — its inverse: (lo, hi) [batch, m, inner] -> y [batch, n_out, inner], n_out = 2 m - L + 2 or one less (the reference's
 *   crop, src/ptwt/_util.py:231-244).
 * mifwt_tap_correlate_planes — mifwt_tap_correlate's reduction on operands [batch, rows, columns] (columns contiguous; batch / row strides in
 *   elements): along = 1: out[t] += sum a[b, r, k] b_ext[b, r, 2k + c0 + sgn t] (a: [batch, R, M], b: [batch, R, N]);
 *   along = 0: out[t] += sum a[b, k, c] b_ext[b, 2k + c0 + sgn t, c] (a: [batch, M, C], b: [batch, N, C]).  L <= 32, f32 / f64. */
int mifwt_dwt1_fwd_outer(int dtype, int64_t batch, int64_t n, int64_t inner, const void* x, int64_t x_batch_stride, int64_t x_axis_stride, void* lo_out,
                         void* hi_out, int64_t out_batch_stride, int64_t out_axis_stride, int mode, int filt_len, const double* dec_lo,
                         const double* dec_hi, const double* d_dec_lo, const double* d_dec_hi, void* stream);
int mifwt_dwt1_inv_outer(int dtype, int64_t batch, int64_t m, int64_t n_out, int64_t inner, const void* lo_in, int64_t lo_batch_stride,
                         int64_t lo_axis_stride, const void* hi_in, int64_t hi_batch_stride, int64_t hi_axis_stride, void* y, int64_t y_batch_stride,
                         int64_t y_axis_stride, int filt_len, const double* rec_lo, const double* rec_hi, const double* d_rec_lo,
                         const double* d_rec_hi, void* stream);
int mifwt_tap_correlate_planes(int dtype, int along, int64_t batch, int64_t a_rows, int64_t a_cols, int64_t b_rows, int64_t b_cols, const void* a,
                               int64_t a_batch_stride, int64_t a_row_stride, const void* b, int64_t b_batch_stride, int64_t b_row_stride,
                               int filt_len, int c0, int sgn, int mode, double* out, void* stream);

/* TWO consecutive 2-D analysis levels in one launch — two trips of the reference's level loop
 * (src/ptwt/conv_transform_2.py:142-149) whose intermediate approximation never reaches HBM: a pyramid returns only the
 * detail bands of a level that is not the last (conv_transform_2.py:150-156), so the write + re-read of that
 * approximation is traffic the per-level seam cannot avoid.  d1 / d2 describe the two levels exactly as two
 * mifwt_dwt_fwd calls would (d2->sig_extent == d1->coef_extent; d1's approx_stride and d2's sig_stride are ignored).
 *   details1  HOST array of 3 device ptrs: level-1 bands ad, da, dd     approx2 / details2: the level-2 bands
 * Results are bit-identical to the two per-level calls.  mifwt_dwt2_fwd_pair_supported() says (1 / 0) whether this
 * build serves the pair (f32, even L <= 8, any mode but periodic, unit innermost strides, level-1 plane at least
 * 64 columns x L + 6 rows); the call itself returns MIFWT_ERR_UNSUPPORTED otherwise and launches nothing. */
int mifwt_dwt2_fwd_pair_supported(const mifwt_level_desc* d1, const mifwt_level_desc* d2);
int mifwt_dwt2_fwd_pair(const mifwt_level_desc* d1, const mifwt_level_desc* d2, const void* x, void* const* details1,
                        void* approx2, void* const* details2, const double* dec_lo, const double* dec_hi, void* stream);

/* SEVERAL consecutive 2-D analysis levels in one launch — `nlevels` trips of the reference's level loop
 * (src/ptwt/conv_transform_2.py:142-149); none of the approximations in between reaches HBM (a pyramid returns only the detail
 * bands of a level that is not the last, conv_transform_2.py:150-156).  descs[l] describes fused level l exactly as a
 * mifwt_dwt_fwd call would (descs[l]->sig_extent == descs[l-1]->coef_extent; approx_stride of every level but the last and
 * sig_stride of every level but the first are ignored).
 *   details  HOST array of nlevels HOST arrays of 3 device ptrs: bands ad, da, dd of fused level l
 *   approx   band aa of the last fused level
 * Same sums as nlevels mifwt_dwt_fwd calls (summation order differs: agreement to rounding, not bit for bit).  Two kernels:
 *   (1) kernel id 16, up to THREE levels, rows streamed through registers and LDS rings: f32, even L <= 8, modes zero / constant /
 *       reflect / symmetric, unit innermost strides (input rows of any length and alignment), every fused plane at least 2 L
 *       samples per axis; in auto mode (MIFWT_OPT_PYRAMID_MODE 0) only for planes of 448 .. ~2560 columns (one or two column groups),
 *       where a workgroup streams whole rows; the three detail planes of a level within 1 GiB of one another;
 *   (2) kernel id 20, up to EIGHT levels — the whole pyramid — of planes small enough to live in LDS (the plane and its
 *       horizontally filtered image, both with their boundary extension, <= 160 KB: 128 x 128 up to 12 taps), a workgroup per
 *       image at a time: f32, even L <= 20, every boundary mode, unit innermost strides; in auto mode planes that keep a
 *       CU's LDS to themselves only from 112 KB of LDS images and 512 images upwards (MIFWT_OPT_PYRAMID_MODE 3 lifts that).
 * mifwt_dwt2_fwd_pyramid_supported says which one serves the call (0 none, 1, 2); MIFWT_ERR_UNSUPPORTED otherwise, nothing launched. */
int mifwt_dwt2_fwd_pyramid_supported(int nlevels, const mifwt_level_desc* const* descs);
int mifwt_dwt2_fwd_pyramid(int nlevels, const mifwt_level_desc* const* descs, const void* x, void* const* const* details, void* approx,
                           const double* dec_lo, const double* dec_hi, void* stream);
/* Kernel (1) runs PERSISTENT workgroups: the rows of the last fused level of all images, laid end to end, are cut into one chunk per
 * workgroup (one workgroup per CU and column group; chunks of equal modelled time), a workgroup runs the parts of images in its chunk
 * one after the other (a part that starts inside an image streams a prologue of (2^nlevels - 1)(L - 2) input rows first).  Results do
 * not depend on the cut.  mifwt_dwt2_fwd_pyramid_schedule writes the cuts of a call into wg_start[0 .. n] (global row indices,
 * wg_start[0] = 0, wg_start[n] = batch x rows) and returns n — diagnostics and tests; MIFWT_ERR_UNSUPPORTED where kernel (1) does not
 * serve the call, MIFWT_ERR_BADARG if `capacity` < n + 1. */
int mifwt_dwt2_fwd_pyramid_schedule(int nlevels, const mifwt_level_desc* const* descs, unsigned int* wg_start, int capacity);

/* Plan of the SLAB form of kernel id 24 for one 3-D analysis level (eight / ten taps, f32, rows of at most 128 samples;
 * csrc/mifwt_dwt3_fwd_slab.hip — one level of wavedec3 / fswavedec3, src/ptwt/conv_transform_3.py:121-141) — diagnostics and tests:
 * out[0 .. 11] = output rows of a slab, slabs per volume, compute waves of a workgroup, floats of a staged row, rows per 1-KiB
 * request, staged rows of a slice, (low, high) pairs of a row of the filtered image, pad samples of a row, depth segments, output
 * slices per segment, bytes of LDS, 1 if the default route takes this form for the level (else 0).  Returns 12; MIFWT_ERR_UNSUPPORTED
 * where the form does not apply, MIFWT_ERR_BADARG if `capacity` < 12. */
int mifwt_dwt3_fwd_slab_plan(const mifwt_level_desc* desc, int* out, int capacity);

/* SEVERAL levels of a 2-D reconstruction in one launch — trips of waverec2's level loop (src/ptwt/conv_transform_2.py:222-249);
 * the running approximation never reaches HBM.
 * descs[0] describes the COARSEST level, descs[nlevels-1] the finest, each exactly as a mifwt_dwt_inv call would: coef_extent = the
 * level's coefficient extents, detail_stride its bands' strides; approx_stride counts for descs[0] only (the coarsest approximation),
 * sig_extent / sig_stride for the last one only (y).  The output of level l is cropped to descs[l+1]->coef_extent (which must not
 * exceed 2 M - L + 2 per axis): the reference's trims (conv_transform_2.py:240-247) and the separable containers' crop
 * (separable_conv_transform.py:94-97) are both that.
 *   approx   the coarsest approximation        details  HOST array of nlevels HOST arrays of 3 device ptrs: bands ad, da, dd
 * Same sums as nlevels mifwt_dwt_inv calls (summation order differs: agreement to rounding).  Two kernels:
 *   (1) kernel id 21, EVERY level (up to eight) of a plane small enough to live in LDS: f32, even L <= 20, dense coefficient planes
 *       (row stride = width), the finest level's coefficients and its vertically synthesised image <= 160 KB (128 x 128 outputs for 8
 *       taps); in auto mode planes that keep a CU's LDS to themselves only from 128 KB of LDS images and 512 images upwards
 *       (MIFWT_OPT_PYRAMID_MODE 3 lifts that);
 *   (2) kernel id 22, up to THREE levels of a big plane, coefficient rows streamed through LDS rings (a caller with more levels runs the
 *       coarser ones first and hands their output over as `approx`): f32, even L <= 10, unit innermost strides, the three detail bands
 *       of a level sharing their strides (any row / image stride, any alignment), output planes of at least 32 rows whose rows fit a
 *       workgroup (about 1500 columns); in auto mode (MIFWT_OPT_PYRAMID_MODE 0) planes from 384 columns on.
 * mifwt_dwt2_inv_pyramid_supported says which one serves the call (0 none, 1, 2; MIFWT_OPT_PYRAMID_MODE 2 switches both off);
 * MIFWT_ERR_UNSUPPORTED otherwise, nothing launched. */
int mifwt_dwt2_inv_pyramid_supported(int nlevels, const mifwt_level_desc* const* descs);
int mifwt_dwt2_inv_pyramid(int nlevels, const mifwt_level_desc* const* descs, const void* approx, const void* const* const* details, void* y,
                           const double* rec_lo, const double* rec_hi, void* stream);

/* TWO consecutive 2-D synthesis levels in one launch — two trips of waverec2's level loop
 * (src/ptwt/conv_transform_2.py:222-249); the approximation between them (the coarser level's cropped output) never
 * reaches HBM.  d2 describes the COARSER level, d1 the finer one, exactly as two mifwt_dwt_inv calls would
 * (d2->sig_extent == d1->coef_extent; d2's sig_stride and d1's approx_stride are ignored).
 *   approx2 / details2  the coarser level's bands      details1  HOST array of 3 device ptrs: finer bands ad, da, dd
 * Results are bit-identical to the two per-level calls.  f32, even L <= 8, unit innermost strides, output plane >= 64 x 64
 * (mifwt_dwt2_inv_pair_supported says 1 / 0); MIFWT_ERR_UNSUPPORTED otherwise, nothing launched. */
int mifwt_dwt2_inv_pair_supported(const mifwt_level_desc* d2, const mifwt_level_desc* d1);
int mifwt_dwt2_inv_pair(const mifwt_level_desc* d2, const mifwt_level_desc* d1, const void* approx2, const void* const* details2,
                        const void* const* details1, void* y, const double* rec_lo, const double* rec_hi, void* stream);

/* The DEEP levels of a 1-D decomposition in one launch — the trailing trips of wavedec's level loop
 * (src/ptwt/conv_transform.py:133-140).  Below a few thousand samples per row a level is launch latency, not work; here one
 * workgroup per row parks the row in LDS and runs `nlevels` levels on it.  Rows of contiguous samples (row strides in
 * elements), f32 / f64, even filt_len <= 32, any boundary mode, n <= mifwt_dwt1_fwd_tail_max_n(dtype), 2 <= nlevels <= 24.
 *   details  HOST array of nlevels device pointers: detail coefficients of fused level l, [rows, floor((n_l + L - 1) / 2)]
 *   approx   the last level's approximation
 * Same sums as nlevels mifwt_dwt_fwd calls (summation order differs: agreement to rounding, not bit for bit).
 * MIFWT_ERR_UNSUPPORTED outside the envelope, nothing launched. */
int mifwt_dwt1_fwd_tail_max_n(int dtype);
int mifwt_dwt1_fwd_tail(int dtype, int filt_len, int mode, int64_t rows, int64_t n, int nlevels, const void* x, int64_t x_row_stride,
                        void* approx, int64_t approx_row_stride, void* const* details, const int64_t* detail_row_strides,
                        const double* dec_lo, const double* dec_hi, void* stream);

/* SEVERAL levels of a 1-D decomposition in one launch, a CHUNK of a row per workgroup — the leading trips of wavedec's level
 * loop (src/ptwt/conv_transform.py:133-140) for rows of at least 4096 samples (longer than one workgroup's LDS or not: the
 * one-workgroup-per-row launch is a latency chain; few rows get smaller chunks, about one workgroup per CU; the two end pieces may
 * be the whole row): a workgroup owns a chunk of a row plus the
 * (L - 2)(2^K - 1) halo samples its K levels consume; the approximations between the levels stay in LDS.  Same arguments as
 * mifwt_dwt1_fwd_tail; f32, even filt_len <= 20, any boundary mode.
 * mifwt_dwt1_fwd_long_levels answers how many of `want` levels one launch fuses for this geometry (it stops where the halo
 * would exceed a twelfth of a chunk; 0 = not served); mifwt_dwt1_fwd_long must be called with exactly that count, MIFWT_ERR_UNSUPPORTED otherwise, nothing
 * launched.  Agreement with per-level calls to rounding. */
int mifwt_dwt1_fwd_long_levels(int dtype, int filt_len, int mode, int64_t rows, int64_t n, int want);
int mifwt_dwt1_fwd_long(int dtype, int filt_len, int mode, int64_t rows, int64_t n, int nlevels, const void* x, int64_t x_row_stride,
                        void* approx, int64_t approx_row_stride, void* const* details, const int64_t* detail_row_strides,
                        const double* dec_lo, const double* dec_hi, void* stream);

/* The COARSE levels of a 1-D reconstruction in one launch — the leading trips of waverec's level loop
 * (src/ptwt/conv_transform.py:184-199: stack + conv_transpose1d(stride 2) + crop per level), mirror of mifwt_dwt1_fwd_tail.
 *   approx   coarsest approximation [rows, m]       details  HOST array of nlevels device ptrs, coarsest first: [rows, m_l]
 *   out_len  HOST array: output samples of fused level l = 2 m_l - L + 2 - t, t in {0, 1} (the reference's end-crop,
 *            src/ptwt/_util.py:231-244); m_{l+1} = out_len[l]
 *   y        output of the last fused level [rows, out_len[nlevels - 1]]
 * f32 / f64, even filt_len <= 32, every out_len <= mifwt_dwt1_fwd_tail_max_n(dtype), 2 <= nlevels <= 24. */
int mifwt_dwt1_inv_tail(int dtype, int filt_len, int64_t rows, int64_t m, int nlevels, const void* approx, int64_t approx_row_stride,
                        const void* const* details, const int64_t* detail_row_strides, const int32_t* out_len, void* y,
                        int64_t y_row_stride, const double* rec_lo, const double* rec_hi, void* stream);

/* The FINEST levels of a 1-D reconstruction in one launch, a chunk of the output row per workgroup — the trailing trips of
 * waverec's level loop (src/ptwt/conv_transform.py:184-199) once a level's output no longer fits into one workgroup's LDS
 * (mirror of mifwt_dwt1_fwd_long; the coarse levels before it are mifwt_dwt1_inv_tail's).
 *   m        HOST array of nlevels + 1 ints: m[s] = coefficients per row entering fused step s (coarsest first) — the length
 *            of approx for s = 0, of details[s] for every s — and m[s + 1] = 2 m[s] - L + 2 - t its output length (t in {0, 1}:
 *            the reference's end-crop, src/ptwt/_util.py:231-244); m[nlevels] = samples per row of y
 *   approx   [rows, m[0]]     details  HOST array of nlevels device ptrs, coarsest first: [rows, m[s]]     y  [rows, m[nlevels]]
 * f32 / f64, even filt_len <= 20, 2 <= nlevels <= 8 with (L/2) 2^nlevels below a twelfth of a chunk (8 K f32 / 4 K f64 samples;
 * smaller for few short rows), output rows of at least 1024 samples (mifwt_dwt1_inv_long_supported says 1 / 0); MIFWT_ERR_UNSUPPORTED otherwise, nothing
 * launched.  Agreement with per-level calls to rounding.  Kernel id 18. */
int mifwt_dwt1_inv_long_supported(int dtype, int filt_len, int64_t rows, int nlevels, const int32_t* m);
int mifwt_dwt1_inv_long(int dtype, int filt_len, int64_t rows, int nlevels, const int32_t* m, const void* approx, int64_t approx_row_stride,
                        const void* const* details, const int64_t* detail_row_strides, void* y, int64_t y_row_stride,
                        const double* rec_lo, const double* rec_hi, void* stream);

/* Diagnostic: the launch geometry mifwt_dwt1_fwd_long (inverse = 0: mode, n, nlevels = the `want` argument; m ignored) or
 * mifwt_dwt1_inv_long (inverse = 1: nlevels, m; mode, n ignored) would use: out6 = {levels, chunk, nchunks, end_l, end_r, cap}
 * (chunk: level-K outputs per interior workgroup / output samples per workgroup; end_l, end_r: level-K outputs of the two end
 * pieces, analysis only; cap: floats of LDS buffer A).  Returns 1, or 0 when the geometry is not served. */
int mifwt_dwt1_long_plan(int inverse, int dtype, int filt_len, int mode, int64_t rows, int64_t n, int nlevels, const int32_t* m, int32_t* out6);

/* Adjoints (transposes) of the two level maps, for reverse-mode differentiation.  The reference gets them from
 * ATen autograd through F.pad / _pad_symmetric + F.conv{1,2,3}d and torch.stack + F.conv_transpose{1,2,3}d
 * (same call sites as above); here they are explicit entry points that take the SAME descriptor as the
 * forward call they differentiate.
 *   mifwt_dwt_fwd_adjoint: g_x = A^T (g_approx, g_details), A = the analysis level incl. its boundary extension
 *       (the halo of the transposed convolution is folded back through the boundary index map).
 *   mifwt_dwt_inv_adjoint: (g_approx, g_details) = S^T g_y, S = the (cropped) synthesis level.
 * Taps are the forward call's taps (dec_* resp. rec_*), PyWavelets order. */
int mifwt_dwt_fwd_adjoint(const mifwt_level_desc* desc, const void* g_approx, const void* const* g_details, void* g_x,
                          const double* dec_lo, const double* dec_hi, void* workspace, size_t workspace_bytes,
                          void* stream);
int mifwt_dwt_inv_adjoint(const mifwt_level_desc* desc, const void* g_y, void* g_approx, void* const* g_details,
                          const double* rec_lo, const double* rec_hi, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Stationary (undecimated) transform levels — ptwt.swt / ptwt.iswt, src/ptwt/stationary_transform.py:95-107
 * (_circular_pad + F.conv1d(stride 1, dilation) + split) and :142-156 (stack + _circular_pad +
 * F.conv_transpose1d(groups 2, dilation) + mean).  `rows` independent rows of `n` contiguous samples, row strides in
 * elements, dilation = 2^level_index, periodic extension as an index map.  `scale` multiplies the result: 1 for swt,
 * 0.5 for iswt (the reference's mean over the two reconstructions); with reversed taps and the other scale each
 * call is the adjoint of the other (backward passes).  Even filt_len <= MIFWT_MAX_FILT (2..20 unrolled, longer
 * filters through a run-time tap loop), f32 / f64 / f16 / bf16.
 *   fwd: lo/hi[n] = scale * sum_m dec_lo/hi[m] x[(n + D (L/2 - m)) mod N]
 *   inv: y[n]     = scale * sum_j rec_lo[j] a[(n + D (L/2 - 1 - j)) mod N] + rec_hi[j] d[(same)] */
int mifwt_swt_fwd(int dtype, int filt_len, int64_t rows, int64_t n, int64_t dilation, const void* x, int64_t x_row_stride,
                  void* lo, void* hi, int64_t lo_row_stride, int64_t hi_row_stride, const double* dec_lo,
                  const double* dec_hi, double scale, void* stream);
int mifwt_swt_inv(int dtype, int filt_len, int64_t rows, int64_t n, int64_t dilation, const void* a, const void* d,
                  int64_t a_row_stride, int64_t d_row_stride, void* y, int64_t y_row_stride, const double* rec_lo,
                  const double* rec_hi, double scale, void* stream);

/* 2-D stationary levels (swt2 / iswt2 of the package: the level above along both axes of a plane, pywt.swt2 with trim_approx=True,
 * norm=False) in ONE launch per level that reads its input planes once and writes its outputs once (kernel ids 34 / 35,
 * csrc/mifwt_swt2.hip: a walk down the a-trous lattice with a register ring of L row pairs; no intermediate plane, no transpose).
 * `images` planes of H rows of W contiguous samples; every plane has its own image and row stride in elements (level j + 1 can read
 * the cA plane of level j's buffer, slices need no copy); outputs must not overlap inputs.  Periodic in both axes with any number of
 * wraps (any H, W >= 1, any dilation >= 1).  row_* filter along W (axis -1), col_* along H (axis -2); `scale` multiplies the result: 1
 * for swt2, 0.25 for iswt2; with all four filters reversed and the same scale each call is the adjoint of the other.
 *   fwd: p_lo/hi[r][n] = sum_t row_lo/hi[t] x[r][(n + D (L/2 - t)) mod W],   bands[0..3] = cA, cH, cV, cD with
 *        cA = scale sum_m col_lo[m] p_lo[(r + D (L/2 - m)) mod H][n], cH = (col_hi, p_lo), cV = (col_lo, p_hi), cD = (col_hi, p_hi)
 *   inv: bands[0..3] = cA, cH, cV, cD;  U[r][n] = sum_t row_lo[t] cA[r][(n + D (L/2 - 1 - t)) mod W] + row_hi[t] cV[r][..],
 *        V likewise from (cH, cD),  y[r][n] = scale sum_m col_lo[m] U[(r + D (L/2 - 1 - m)) mod H][n] + col_hi[m] V[..][n]
 * LIMIT: the ring lives in registers, so only the unrolled lengths exist: even filt_len 2 .. 20, f32 / f64, extents and
 * dilation * filt_len below 2^28.  mifwt_swt2_supported answers 1 where the two entries run and 0 where they answer
 * MIFWT_ERR_UNSUPPORTED (longer filters, f16): the caller then composes the level from mifwt_swt_fwd / mifwt_swt_inv.
 * MIFWT_OPT_ROWS_PER_CHUNK > 0 overrides the lattice rows per wave. */
int mifwt_swt2_supported(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation);
int mifwt_swt2_fwd(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation, const void* x,
                   int64_t x_image_stride, int64_t x_row_stride, void* const* bands, const int64_t* band_image_strides,
                   const int64_t* band_row_strides, const double* row_lo, const double* row_hi, const double* col_lo,
                   const double* col_hi, double scale, void* stream);
int mifwt_swt2_inv(int dtype, int filt_len, int64_t images, int64_t H, int64_t W, int64_t dilation, const void* const* bands,
                   const int64_t* band_image_strides, const int64_t* band_row_strides, void* y, int64_t y_image_stride,
                   int64_t y_row_stride, const double* row_lo, const double* row_hi, const double* col_lo, const double* col_hi,
                   double scale, void* stream);

/* 3-D stationary levels (swt3 / iswt3 of the package: the 1-D level above along the three axes of a volume, pywt.swtn with
 * trim_approx=True, norm=False by construction) in ONE launch per level that writes every output once and keeps no intermediate
 * volume in global memory (kernel ids 36 / 37, csrc/mifwt_swt3.hip: a workgroup walks down the a-trous lattice of slices; axis -1
 * from global memory into an LDS tile of lattice rows, axis -2 from LDS, axis -3 in a register ring).  `volumes` volumes of Dz slices
 * of H rows of W contiguous samples; every operand has its own volume, slice and row stride in elements (level j + 1 can read plane 0
 * of level j's [B, 8, Dz, H, W] buffer, slices need no copy); outputs must not overlap inputs.  Periodic in all three axes with any
 * number of wraps (any Dz, H, W >= 1, any dilation >= 1).  taps[0..5] = w_lo, w_hi (along W, axis -1), h_lo, h_hi (along H, axis
 * -2), z_lo, z_hi (along Dz, axis -3), filt_len doubles each.  Band q = 4 [axis -3 high] + 2 [axis -2 high] + [axis -1 high]: aaa,
 * aad, ada, add, daa, dad, dda, ddd.  `scale` multiplies the result: 1 for swt3, 0.125 for iswt3; with all six filters reversed and
 * the same scale each call is the adjoint of the other.
 *   fwd: bands[q][s][r][n] = scale sum_k z[k] sum_m h[m] sum_t w[t] x[(s + D (L/2 - k)) mod Dz][(r + D (L/2 - m)) mod H][(n + D (L/2 - t)) mod W]
 *        with (z, h, w) the low- or high-pass filter of each axis as the bits of q say
 *   inv: y[s][r][n] = scale sum_q sum_k z[k] sum_m h[m] sum_t w[t] bands[q][(s + D (L/2 - 1 - k)) mod Dz][(r + D (L/2 - 1 - m)) mod H][(n + D (L/2 - 1 - t)) mod W]
 * LIMIT: compile-time lengths only: even filt_len 2 .. 10, f32 / f64, extents and dilation * filt_len below 2^28.
 * mifwt_swt3_supported answers 1 where the two entries run and 0 where they answer MIFWT_ERR_UNSUPPORTED (longer filters, f16): the
 * caller then composes the level from mifwt_swt2_* and mifwt_swt_*.  MIFWT_OPT_ROWS_PER_CHUNK > 0 overrides the lattice slices per
 * workgroup.  mifwt_swt3_plan (diagnostics and tests; host code, launches nothing) writes the work split of such a launch into
 * out[0 .. MIFWT_SWT3_PLAN_INTS): slice residues, row residues, slice segments, lattice slices per segment, row tiles, column
 * strips, tile rows RT, tile rows per lane RW, columns per lane E, LDS bytes, threads per workgroup; a workgroup per (volume, slice
 * residue, row residue, segment, row tile, strip), a strip = 64 E columns.  Returns the number of ints written or an error. */
#define MIFWT_SWT3_PLAN_INTS 11
int mifwt_swt3_supported(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation);
int mifwt_swt3_fwd(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation, const void* x,
                   int64_t x_volume_stride, int64_t x_slice_stride, int64_t x_row_stride, void* const* bands,
                   const int64_t* band_volume_strides, const int64_t* band_slice_strides, const int64_t* band_row_strides,
                   const double* const* taps, double scale, void* stream);
int mifwt_swt3_inv(int dtype, int filt_len, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation,
                   const void* const* bands, const int64_t* band_volume_strides, const int64_t* band_slice_strides,
                   const int64_t* band_row_strides, void* y, int64_t y_volume_stride, int64_t y_slice_stride, int64_t y_row_stride,
                   const double* const* taps, double scale, void* stream);
int mifwt_swt3_plan(int dtype, int filt_len, int inverse, int64_t volumes, int64_t Dz, int64_t H, int64_t W, int64_t dilation, int* out,
                    int capacity);

/* BOUNDARY-WAVELET levels — the padding-free transforms ptwt.MatrixWavedec / MatrixWaverec (src/ptwt/matmul_transform.py:409-430: pad one
 * sample if odd + torch.sparse.mm(A, x) + split; :679-703: cat + torch.sparse.mm(S, c) + drop the pad sample) and, in their separable
 * form, MatrixWavedec2 / MatrixWaverec2 (src/ptwt/matmul_transform_2.py:514-529: A_rows X A_cols^T through two transposes + splits;
 * :799-840: the cats, S_rows C S_cols^T, crops).  The N x N level matrix (N = 2 M) is never formed: row m of a band is
 *     y[m] = sum_t f[t] x[2 m + L/2 - t]                                   (f = lo / hi below, zero extension never reached)
 * except for the first n_top = ceil((L-2)/4) and the last n_bot = floor(L/4) rows of each band, whose orthogonalised coefficients come from
 * a table: one fused launch per level (kernel ids 26 / 27: f32 / f64, even L <= 20, 1 or 2 transformed axes, unit innermost strides, every
 * axis at least 2 (L-1) samples so that the two ends do not overlap).
 *   desc      as for mifwt_dwt_fwd, with sig_extent the REAL extent (may be odd) and coef_extent = ceil(sig_extent / 2) per axis; an odd
 *             extent has one virtual sample at its end whose value `mode` defines (the reference's odd_coeff_padding_mode).  Synthesis
 *             accepts sig_extent in {2 M, 2 M - 1} and computes only those samples; it ignores `mode`.
 *   lo / hi   HOST taps, PyWavelets order: dec_lo / dec_hi for mifwt_bwt_fwd, rec_lo / rec_hi for mifwt_bwt_inv (which reverses them: the
 *             rows of S^T are built from the reversed filters, matmul_transform.py:111-118)
 *   tables    boundary rows of the same bank on the DEVICE, float64 [2 bands][max(n_top + n_bot, 1)][L]: rows 0 .. n_top-1 hold the top
 *             rows over columns 0 .. L-1 (last entry 0), the others the bottom rows over columns N-L .. N-1 (first entry 0).  They do not
 *             depend on N, so one table serves every level and every axis; the kernels read it once per workgroup that owns an end.
 * mifwt_bwt_fwd applies the rows of the bank (lo, hi, tables), mifwt_bwt_inv the TRANSPOSED bank of (reversed lo, reversed hi, tables).
 * Adjoints therefore need no entry points of their own: the adjoint of an analysis level is mifwt_bwt_inv with (reversed dec_lo, reversed
 * dec_hi, the ANALYSIS tables), the adjoint of a synthesis level mifwt_bwt_fwd with (reversed rec_lo, reversed rec_hi, the SYNTHESIS
 * tables) and mode zero — for biorthogonal filters S != A^T, so an adjoint never borrows the other direction's tables.  (The gradient of
 * the virtual sample of an odd extent is folded back by the caller: run the adjoint over 2 M samples, add column 2 M - 1 to its source.)
 * mifwt_bwt_supported / mifwt_bwt_kernel_id are decided on the host: 1 / the kernel id where the fused kernels serve the level, 0 /
 * MIFWT_ERR_UNSUPPORTED where they do not (the calls then launch nothing), MIFWT_ERR_BADARG for inconsistent extents.
 * mifwt_bwt_axis_fwd / _inv: ONE axis of a level through a run-time tap loop (ids 28 / 29): arrays [outer, n, inner] with (outer, axis,
 * inner) strides in elements, even L <= MIFWT_MAX_FILT, f32 / f64, n (real extent, may be odd) with 2 ceil(n/2) >= 2 (L-1). */
#define MIFWT_KID_BWT_FWD 26
#define MIFWT_KID_BWT_INV 27
#define MIFWT_KID_BWT_AXIS_FWD 28
#define MIFWT_KID_BWT_AXIS_INV 29
typedef struct mifwt_bwt_tables {
  const double* rows; /* DEVICE pointer, layout above */
  int32_t n_top, n_bot;
} mifwt_bwt_tables;
int mifwt_bwt_supported(const mifwt_level_desc* desc, int direction);
int mifwt_bwt_kernel_id(const mifwt_level_desc* desc, int direction);
int mifwt_bwt_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream);
int mifwt_bwt_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                  const mifwt_bwt_tables* tables, void* stream);
int mifwt_bwt_axis_fwd(int dtype, int filt_len, int mode, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides,
                       void* lo_out, const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi,
                       const mifwt_bwt_tables* tables, void* stream);
int mifwt_bwt_axis_inv(int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* lo_in, const int64_t* lo_strides,
                       const void* hi_in, const int64_t* hi_strides, void* y, const int64_t* y_strides, const double* lo, const double* hi,
                       const mifwt_bwt_tables* tables, void* stream);

/* THREE transformed axes (ptwt.MatrixWavedec3 / MatrixWaverec3, src/ptwt/matmul_transform_3.py: the level operator applied along width,
 * height and depth): one fused launch per level (kernel ids 30 / 31, csrc/mifwt_bwt3.hip) that reads the volume once and writes the eight
 * bands once.  ENVELOPE: f32 / f64, even L <= 8, unit innermost strides, every axis at least 2 (L-1) samples.
 *   desc      ndim = 3; extents (depth, height, width) as for mifwt_bwt_fwd; `details` = 7 pointers that share detail_stride, detail
 *             s-1 = band s with bit 2 of s = high-pass along depth, bit 1 along height, bit 0 along width (the order of mifwt_dwt_fwd)
 * Tap order, table layout (the same struct, one table for all three axes) and the adjoint rules are those of mifwt_bwt_fwd / _inv.
 * mifwt_bwt3_supported / mifwt_bwt3_kernel_id: 1 / 30 (direction 0) or 31 (direction 1) where the fused kernel serves the level;
 * 0 / MIFWT_ERR_UNSUPPORTED where it does not (L above the envelope, f16, a non-unit innermost stride, an axis shorter than 2 (L-1),
 * extents beyond the kernels' index range; mifwt_bwt3_fwd / _inv then launch nothing and return MIFWT_ERR_UNSUPPORTED: run the axis passes
 * 28 / 29); MIFWT_ERR_BADARG for ndim != 3, an odd or too long L, coef_extent != ceil(sig_extent / 2), an axis shorter than L, an unknown
 * dtype or mode, or null pointers.  mifwt_bwt_supported / mifwt_bwt_kernel_id keep declining ndim == 3. */
#define MIFWT_KID_BWT3_FWD 30
#define MIFWT_KID_BWT3_INV 31
int mifwt_bwt3_supported(const mifwt_level_desc* desc, int direction);
int mifwt_bwt3_kernel_id(const mifwt_level_desc* desc, int direction);
int mifwt_bwt3_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                   const mifwt_bwt_tables* tables, void* stream);
int mifwt_bwt3_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                   const mifwt_bwt_tables* tables, void* stream);

/* A SUBTREE of a 1-D boundary-wavelet PACKET tree per launch (kernel ids 32 / 33, csrc/mifwt_bwt_tree.hip; ptwt.WaveletPacket with
 * mode="boundary").  A packet node of h samples splits into two nodes of h / 2, so level s below a row of n samples is the dense span
 * [2^s nodes][n / 2^s] of again n numbers.  One workgroup keeps a row and its next level in LDS and computes `nlevels` levels.
 *   rows, n     the rows (nodes of the tree folded into the batch) and their length
 *   levels      HOST array of `nlevels` DEVICE pointers to dense [rows, n] buffers.  mifwt_bwt_tree_fwd: levels[i] = level i + 1 below the
 *               rows (written).  mifwt_bwt_tree_inv: levels[i] = level i, levels[0] the rows themselves (all written; `leaves` = level
 *               nlevels, dense [rows, n], read).
 *   x           rows of unit sample stride, `x_row_stride` >= n elements apart
 *   lo / hi / tables   as for mifwt_bwt_fwd (dec_* and the analysis tables) / mifwt_bwt_inv (rec_* and the synthesis tables)
 * mifwt_bwt_tree_levels: how many consecutive levels ONE launch takes from a node of n samples, at most `max_levels` (0: none; a host
 * decision, no device needed).  Envelope: f32 / f64, even L <= 20, at least two levels, every fused level's input node even and at least
 * 2 (L-1) samples long, n <= 8192 f32 / 4096 f64 samples (two LDS images of 32 KB).  The calls take exactly what that function answers
 * for (n, nlevels); MIFWT_ERR_UNSUPPORTED otherwise (odd n, L > 20, nlevels < 2, f16, ...), nothing launched. */
#define MIFWT_KID_BWT_TREE_FWD 32
#define MIFWT_KID_BWT_TREE_INV 33
int mifwt_bwt_tree_levels(int dtype, int filt_len, int64_t n, int max_levels);
int mifwt_bwt_tree_fwd(int dtype, int filt_len, int64_t rows, int64_t n, int64_t x_row_stride, int nlevels, const void* x,
                       void* const* levels, const double* lo, const double* hi, const mifwt_bwt_tables* tables, void* stream);
int mifwt_bwt_tree_inv(int dtype, int filt_len, int64_t rows, int64_t n, int nlevels, const void* leaves, void* const* levels,
                       const double* lo, const double* hi, const mifwt_bwt_tables* tables, void* stream);

/* PERIODIZED levels — PyWavelets' mode="periodization" (pywt.dwt / pywt.idwt and their N-D forms; the reference has no such mode): an
 * axis of N samples gives ceil(N / 2) coefficients per band, any N >= 1, exactly orthogonal for orthogonal wavelets.  Per axis, L even,
 * taps in PyWavelets order:
 *     extension   N~ = N + (N mod 2);  x~[i] = x[min(i, N - 1)] for 0 <= i < N~ (an odd extent repeats its last sample), then periodic
 *                 with period N~, any number of wraps (N = 1 and N < L are valid)
 *     analysis    M = N~ / 2;  cA[k] = sum_j dec_lo[j] x~[(2 k + L/2 - j) mod N~],  cD likewise with dec_hi,  0 <= k < M
 *     synthesis   y[(2 k + t - L/2 + 1) mod 2 M] += rec_lo[t] cA[k] + rec_hi[t] cD[k],  0 <= k < M, 0 <= t < L  (2 M samples, one more than
 *                 an odd input had, exactly as pywt.idwt)
 * N-D: the 1-D level per transformed axis, separably; band order as everywhere (bit (ndim-1-a) set <=> high-pass along axis a).
 *   desc      as for mifwt_bwt_fwd: sig_extent the REAL extent (may be odd), coef_extent = ceil(sig_extent / 2) per axis (anything else:
 *             MIFWT_ERR_BADARG); `mode` is ignored.  Synthesis accepts sig_extent in {2 M, 2 M - 1} and writes only those samples.
 *   lo / hi   HOST taps, PyWavelets order: dec_lo / dec_hi for mifwt_per_fwd, rec_lo / rec_hi for mifwt_per_inv
 * Adjoints need no entry points of their own: the adjoint of an analysis level is mifwt_per_inv with rec[t] := dec[L-1-t] over N~ samples,
 * after which the caller adds the gradient of the virtual sample N~ - 1 of an odd extent to sample N - 1; the adjoint of a synthesis level
 * is mifwt_per_fwd with dec[j] := rec[L-1-j].
 * Fused kernels (ids 38 / 39, csrc/mifwt_per.hip): f32 / f64, even L from 2 to 20, ndim 1 or 2, unit innermost strides, any extent >= 1: one
 * launch per level, the plane read once and the bands written once.  mifwt_per_supported / mifwt_per_kernel_id are decided on the host:
 * 1 / the kernel id where the fused kernels serve the level, 0 / MIFWT_ERR_UNSUPPORTED where they do not (mifwt_per_fwd / _inv then
 * launch nothing and return MIFWT_ERR_UNSUPPORTED), MIFWT_ERR_BADARG for inconsistent arguments.
 * mifwt_per_axis_fwd / _inv: ONE axis of a level through a run-time tap loop (ids 40 / 41): arrays [outer, n, inner] with (outer, axis,
 * inner) strides in elements, even L <= MIFWT_MAX_FILT, f32 / f64, any n >= 1 (n_out in {2 M, 2 M - 1} for M coefficients). */
#define MIFWT_KID_PER_FWD 38       /* fused level, ndim 1 or 2 */
#define MIFWT_KID_PER_INV 39
#define MIFWT_KID_PER_AXIS_FWD 40  /* one axis, any strides, run-time tap loop */
#define MIFWT_KID_PER_AXIS_INV 41
int mifwt_per_supported(const mifwt_level_desc* desc, int direction);
int mifwt_per_kernel_id(const mifwt_level_desc* desc, int direction);
int mifwt_per_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* lo, const double* hi,
                  void* stream);
int mifwt_per_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* lo, const double* hi,
                  void* stream);
int mifwt_per_axis_fwd(int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides, void* lo_out,
                       const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi, void* stream);
int mifwt_per_axis_inv(int dtype, int filt_len, int64_t outer, int64_t n_out, int64_t inner, const void* lo_in, const int64_t* lo_strides,
                       const void* hi_in, const int64_t* hi_strides, void* y, const int64_t* y_strides, const double* lo, const double* hi,
                       void* stream);

/* VALUE-MAP extension levels — PyWavelets' modes "smooth", "antisymmetric" and "antireflect" (the reference has none of them): the padded
 * level of mode "zero" with the zeros replaced by an extension xe whose samples are weighted sums of source samples, so no index map
 * serves them and `mifwt_mode` does not list them; the entry points take `ext_mode` (MIFWT_EXT_*) next to the descriptor, whose `mode` is
 * ignored.  Per axis of N samples, xe[i] = x[i] for 0 <= i < N and, with floor division,
 *     antisymmetric   q, r = divmod(i, N):    q even: x[r];  q odd: -x[N-1-r]                                       (any N >= 1)
 *     antireflect     q, r = divmod(i, N-1):  q even: x[r] + q (x[N-1] - x[0]);  q odd: -x[N-1-r] + (q+1) x[N-1] - (q-1) x[0];  N = 1: x[0]
 *     smooth          i < 0: x[0] + i (x[1] - x[0]);  i >= N: x[N-1] + (i-N+1) (x[N-1] - x[N-2]);  N = 1: x[0]
 * any number of wraps, no pad check.  L even, taps in PyWavelets order:
 *     analysis    M = floor((N + L - 1) / 2);  cA[k] = sum_j dec_lo[j] xe[2 k + 1 - j],  cD likewise with dec_hi,  0 <= k < M
 *                 (pads of L - 2 on the left and L - 2 + (N mod 2) on the right, as every padded mode)
 *     adjoint     T[i] = sum_k dec_lo[2 k + 1 - i] gA[k] + dec_hi[2 k + 1 - i] gD[k] over -(L-2) <= i < N + L - 2 + (N mod 2);
 *                 g_x[s] = sum_i E[i, s] T[i],  E[i, s] the weight of x[s] in xe[i]
 * N-D: the 1-D level per transformed axis, separably; band order as everywhere (bit (ndim-1-a) set <=> high-pass along axis a).  Synthesis is
 * the padded synthesis (mifwt_dwt_inv), which has no mode.
 *   desc      as for mifwt_per_fwd: sig_extent = N, coef_extent = floor((N + L - 1) / 2) per axis (anything else: MIFWT_ERR_BADARG)
 *   lo / hi   HOST taps dec_lo / dec_hi, PyWavelets order, for the analysis AND its adjoint
 * Fused kernels (ids 42 / 43, csrc/mifwt_ext.hip): f32 / f64, even L from 2 to 20, ndim 1 or 2, unit innermost strides, any extent >= 1: one
 * launch per level, no padded-extent tensor in global memory.  mifwt_ext_supported / mifwt_ext_kernel_id are decided on the host: 1 / the
 * kernel id where the fused kernels serve the level (direction 0 analysis, 1 adjoint), 0 / MIFWT_ERR_UNSUPPORTED where they do not
 * (mifwt_ext_fwd / _adj then launch nothing and return MIFWT_ERR_UNSUPPORTED), MIFWT_ERR_BADARG for inconsistent arguments.
 * mifwt_ext_axis_fwd / _adj: ONE axis of a level through a run-time tap loop (ids 44 / 45): arrays [outer, n, inner] with (outer, axis,
 * inner) strides in elements, even L <= MIFWT_MAX_FILT, f32 / f64, any n >= 1; the coefficient arrays have floor((n + L - 1) / 2) entries. */
#define MIFWT_EXT_SMOOTH 0
#define MIFWT_EXT_ANTISYMMETRIC 1
#define MIFWT_EXT_ANTIREFLECT 2
#define MIFWT_KID_EXT_FWD 42       /* fused analysis level, ndim 1 or 2 */
#define MIFWT_KID_EXT_ADJ 43       /* its adjoint */
#define MIFWT_KID_EXT_AXIS_FWD 44  /* one axis, any strides, run-time tap loop */
#define MIFWT_KID_EXT_AXIS_ADJ 45
int mifwt_ext_supported(const mifwt_level_desc* desc, int ext_mode, int direction);
int mifwt_ext_kernel_id(const mifwt_level_desc* desc, int ext_mode, int direction);
int mifwt_ext_fwd(const mifwt_level_desc* desc, int ext_mode, const void* x, void* approx, void* const* details, const double* lo,
                  const double* hi, void* stream);
int mifwt_ext_adj(const mifwt_level_desc* desc, int ext_mode, const void* g_approx, const void* const* g_details, void* g_x, const double* lo,
                  const double* hi, void* stream);
int mifwt_ext_axis_fwd(int ext_mode, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* x, const int64_t* x_strides,
                       void* lo_out, const int64_t* lo_strides, void* hi_out, const int64_t* hi_strides, const double* lo, const double* hi,
                       void* stream);
int mifwt_ext_axis_adj(int ext_mode, int dtype, int filt_len, int64_t outer, int64_t n, int64_t inner, const void* g_lo, const int64_t* lo_strides,
                       const void* g_hi, const int64_t* hi_strides, void* g_x, const int64_t* x_strides, const double* lo, const double* hi,
                       void* stream);

/* COMPLEX levels — the padded levels of the five index-map modes on INTERLEAVED complex data (complex64 / complex128: pairs (re, im) of
 * float / double), as PyWavelets computes them: the taps are real, so T(a + i b) = T(a) + i T(b), band by band.  desc->dtype names the
 * COMPONENT type, MIFWT_F32 or MIFWT_F64 (a 16-bit storage type: MIFWT_ERR_UNSUPPORTED); every extent and every stride of the descriptor
 * counts COMPLEX elements, and so does every index below.  Per axis, L even, taps in PyWavelets order:
 *     extension   xe[i] = x[s(i)], s the index map of desc->mode (enum mifwt_mode; zero mode: xe[i] = 0 outside) applied to the COMPLEX
 *                 index i, any number of wraps — element i of the pad is a whole element of the signal, never a swapped pair
 *     analysis    M = floor((N + L - 1) / 2);  cA[k] = sum_j dec_lo[j] xe[2 k + 1 - j],  cD likewise with dec_hi,  0 <= k < M
 *     synthesis   y[n] = sum_k rec_lo[n + L - 2 - 2 k] cA[k] + rec_hi[n + L - 2 - 2 k] cD[k],  0 <= n < N, where sig_extent = N is the
 *                 CROPPED output extent, 2 M - L + 2 or one less (anything else: MIFWT_ERR_BADARG); desc->mode is ignored
 * N-D: the 1-D level per transformed axis, separably; band order as everywhere (bit (ndim-1-a) set <=> high-pass along axis a).
 *   desc      sig_extent = N and coef_extent = M per axis as above; mode = enum mifwt_mode for the analysis
 *   lo / hi   HOST taps, real, PyWavelets order: dec_lo / dec_hi for mifwt_cplx_fwd, rec_lo / rec_hi for mifwt_cplx_inv
 * Fused kernels (ids 46 / 47, csrc/mifwt_cplx.hip): even L from 2 to 20, ndim 1 or 2, unit innermost strides, any extent >= 1: one launch
 * per level, no workspace, no atomics (the same input gives the same bits, and the real plane of every output depends on the real plane
 * of the input alone).  mifwt_cplx_supported / mifwt_cplx_kernel_id are decided on the host (direction 0 analysis, 1 synthesis): 1 / the
 * kernel id where the fused kernels serve the level, 0 / MIFWT_ERR_UNSUPPORTED where they do not (ndim 3, L > 20, a non-unit innermost
 * stride; mifwt_cplx_fwd / _inv then launch nothing and return MIFWT_ERR_UNSUPPORTED: filter the two components with the real entry
 * points), MIFWT_ERR_BADARG for inconsistent arguments. */
#define MIFWT_KID_CPLX_FWD 46 /* fused analysis level, ndim 1 or 2 */
#define MIFWT_KID_CPLX_INV 47 /* fused padded synthesis level with its crop */
int mifwt_cplx_supported(const mifwt_level_desc* desc, int direction);
int mifwt_cplx_kernel_id(const mifwt_level_desc* desc, int direction);
int mifwt_cplx_fwd(const mifwt_level_desc* desc, const void* x, void* approx, void* const* details, const double* dec_lo,
                   const double* dec_hi, void* stream);
int mifwt_cplx_inv(const mifwt_level_desc* desc, const void* approx, const void* const* details, void* y, const double* rec_lo,
                   const double* rec_hi, void* stream);

/* THRESHOLDING — pywt.threshold / pywt.threshold_firm over up to mifwt_thresh_max_segments() tensors per launch (csrc/mifwt_thresh.hip).
 * With m = |x| (complex data: the magnitude of the complex number), v the threshold, s the substitute:
 *     MIFWT_THRESH_SOFT     x max(1 - v / m, 0)         (s where m < v, if s != 0)
 *     MIFWT_THRESH_HARD     x if m >= v, else s
 *     MIFWT_THRESH_GARROTE  x max(1 - v^2 / m^2, 0)     (s where m < v, if s != 0)
 *     MIFWT_THRESH_GREATER  x if x >= v, else s         (real data)
 *     MIFWT_THRESH_LESS     x if x <= v, else s         (real data)
 *     MIFWT_THRESH_FIRM     0 for m <= v_lo;  x v_hi (1 - v_lo / m) / (v_hi - v_lo) for v_lo < m <= v_hi;  x for m > v_hi
 * x = 0 gives 0 (no 0 / 0), v_hi == v_lo divides nothing.  Arithmetic in float for MIFWT_F32 / F16 / BF16, in double for MIFWT_F64; `dtype`
 * names the COMPONENT type of complex data (`is_complex`: interleaved pairs; extents and strides count complex elements).
 * A SEGMENT is one tensor: extent[0] x extent[1] rows of extent[2] contiguous elements (stride[2] must be 1; unused outer extents are
 * 1).  Its thresholds are host doubles (value[k]) or, where dvalue[k] is not NULL, DEVICE float64 values read by the kernel (nothing is
 * copied to the host: capturable): element (i0, i1, .) takes dvalue[k][(i0 * extent[1] + i1) / rows_per_value[k]], rows_per_value[k] == 0
 * meaning one value; it must divide the number of rows, and the two of a firm call must nest.  k = 0: the threshold (firm: v_lo), k = 1:
 * firm's v_hi.  The table is copied into the kernel arguments; no device-side table, no workspace in the forward.
 *   mifwt_thresh_fwd  (kernel id 48) y = T(x)
 *   mifwt_thresh_bwd  (kernel id 49, real data) y = g dT/dx from the saved input x and the upstream gradient g, and, for every segment
 *                     and k with gvalue[k] != NULL, gvalue[k][index] = sum of g dT/dv_k over the elements of that index, summed over ALL
 *                     segments of the call that name the same gvalue[k] (hard / greater / less: nothing is written, the gradient is 0).
 *                     `workspace`: 16 bytes per unit of mifwt_thresh_plan (float64 partials, one plain store per workgroup and
 *                     threshold, summed per destination by a second small launch in a fixed order: no atomics, reproducible).
 *   mifwt_thresh_plan (host only) the number of units (workgroup iterations) of the call, and, if unit_start is not NULL, the first unit
 *                     of every segment in unit_start[0 .. nseg] (unit_start[nseg] = the total) — workspace sizing and tests.
 * MIFWT_ERR_BADARG for nseg outside [1, mifwt_thresh_max_segments()], an unknown mode or dtype, a non-unit innermost stride, inconsistent
 * rows_per_value; MIFWT_ERR_UNSUPPORTED for greater / less on complex data, complex 16-bit storage, extents beyond the kernels' index
 * range (2^30 elements per row, 2^31 rows or units); MIFWT_ERR_WORKSPACE for a workspace that is too small.  Nothing is launched then. */
#define MIFWT_THRESH_SOFT 0
#define MIFWT_THRESH_HARD 1
#define MIFWT_THRESH_GARROTE 2
#define MIFWT_THRESH_GREATER 3
#define MIFWT_THRESH_LESS 4
#define MIFWT_THRESH_FIRM 5
#define MIFWT_KID_THRESH_FWD 48 /* thresholding, every segment of the call in one launch */
#define MIFWT_KID_THRESH_BWD 49 /* its backward: g dT/dx and the per-workgroup partials of g dT/dv */
typedef struct mifwt_thresh_seg {
  const void* x;
  void* y;
  const void* g; /* backward only */
  int64_t extent[3];
  int64_t x_stride[3], y_stride[3], g_stride[3]; /* in elements */
  double value[2];
  const double* dvalue[2];
  int64_t rows_per_value[2];
  double* gvalue[2]; /* backward only */
} mifwt_thresh_seg;
int mifwt_thresh_max_segments(void);
int64_t mifwt_thresh_plan(int dtype, int is_complex, const mifwt_thresh_seg* segs, int nseg, int64_t* unit_start);
int mifwt_thresh_fwd(int dtype, int is_complex, int mode, double substitute, const mifwt_thresh_seg* segs, int nseg, void* stream);
int mifwt_thresh_bwd(int dtype, int mode, const mifwt_thresh_seg* segs, int nseg, void* workspace, size_t workspace_bytes, void* stream);

/* ESTIMATORS — the noise level of a detail band (median absolute deviation) and the VisuShrink / BayesShrink thresholds of a coefficient
 * container, written on the device in the form mifwt_thresh_fwd reads (csrc/mifwt_estim.hip).  MIFWT_F32 / MIFWT_F64.
 * A BAND is one tensor: extent[0] x extent[1] rows of extent[2] contiguous elements (stride[2] must be 1; unused outer extents are 1);
 * rows_per_index consecutive rows form one leading index ("image"; 0: the whole band is one), and it must divide the number of rows.
 * An image holds fewer than 2^31 elements.
 *   mifwt_estim_sigma       per image: lo / hi = the order statistics of |x| of rank (c - 1) / 2 and c / 2 (c elements) — exact, the bits
 *                           a sort gives, selected on the bit pattern with the sign cleared — and sigma = (lo + hi) / 2 /
 *                           0.6744897501960817 in float64, rounded once.  order_stats ([images][2]) and sigma ([images]) are of the
 *                           data's type, sigma64 holds the ROUNDED sigma as float64; each may be NULL.  `route` is
 *                           MIFWT_KID_ESTIM_SELECT_LDS (50: one workgroup per image, the image's keys in LDS; at most
 *                           mifwt_estim_lds_capacity(dtype) elements per image) or MIFWT_KID_ESTIM_SELECT_STREAM (51: digit passes over the
 *                           band with integer counters in `workspace`, mifwt_estim_select_workspace bytes, zeroed on the stream).
 *                           mifwt_estim_select_route names the default route (0: an empty band, nothing to launch).
 *   mifwt_estim_stream_plan (host only) the number of digit passes of route 51 and, for a pass in range, its shift and width.
 *   mifwt_estim_thresholds  for up to mifwt_estim_max_segments() bands that share `images`, thr[s][g] (the data's type) and thr64[s][g] (the
 *                           rounded value as float64, what mifwt_thresh_fwd takes as dvalue); either may be NULL.
 *                           MIFWT_ESTIM_VISU (kernel id 53): sigma64[g] * factor; the bands are not read.
 *                           MIFWT_ESTIM_BAYES (kernel id 52): sigma^2 / sqrt(max(mean(x^2) - sigma^2, eps)), eps the machine epsilon of the
 *                           data's type; the sums of x^2 in float64, per workgroup into `workspace` (8 bytes per unit of
 *                           mifwt_estim_moments_plan) and per image in a fixed order by a second launch — no float atomics, reproducible.
 *                           moments, if not NULL, receives the sums ([nseg][images]).
 * Nothing is copied to the host and nothing synchronises: the calls can be captured.  MIFWT_ERR_BADARG for an unknown dtype, route or
 * method, a non-unit innermost stride, inconsistent rows_per_index, bands of other image counts or an empty band in
 * mifwt_estim_thresholds; MIFWT_ERR_UNSUPPORTED beyond the index range (2^30 elements per row, 2^31 rows, 2^31 elements per image) or the
 * LDS capacity; MIFWT_ERR_WORKSPACE for a workspace that is too small.  The estimator launches are not counted by mifwt_launch_count. */
#define MIFWT_KID_ESTIM_SELECT_LDS 50    /* order statistics of |x|, an image's keys resident in LDS */
#define MIFWT_KID_ESTIM_SELECT_STREAM 51 /* order statistics of |x|, streaming digit passes with integer counters */
#define MIFWT_KID_ESTIM_MOMENTS 52       /* sum of x^2 per (band, image) of a container + the BayesShrink thresholds */
#define MIFWT_KID_ESTIM_VISU 53          /* the VisuShrink thresholds from sigma */
#define MIFWT_ESTIM_VISU 0
#define MIFWT_ESTIM_BAYES 1
typedef struct mifwt_estim_band {
  const void* x;
  int64_t extent[3];
  int64_t stride[3]; /* in elements */
  int64_t rows_per_index;
} mifwt_estim_band;
int mifwt_estim_max_segments(void);
int mifwt_estim_lds_capacity(int dtype);
int mifwt_estim_stream_plan(int dtype, int pass, int* shift, int* width);
int mifwt_estim_select_route(int dtype, const mifwt_estim_band* band, int force_stream);
size_t mifwt_estim_select_workspace(int dtype, const mifwt_estim_band* band, int route);
int mifwt_estim_sigma(int dtype, const mifwt_estim_band* band, int route, void* order_stats, void* sigma, double* sigma64, void* workspace,
                      size_t workspace_bytes, void* stream);
int64_t mifwt_estim_moments_plan(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images);
int mifwt_estim_thresholds(int dtype, int method, const mifwt_estim_band* segs, int nseg, int64_t images, const double* sigma64,
                           double factor, void* thr, double* thr64, double* moments, void* workspace, size_t workspace_bytes, void* stream);

/* NODE COSTS — the additive cost of every node of a wavelet packet tree, what the Coifman-Wickerhauser best-basis search compares
 * (csrc/mifwt_cost.hip).  MIFWT_F32 / MIFWT_F64.  A SEGMENT is a band as above whose rows_per_index consecutive rows form one NODE (0:
 * the whole band is one node); every segment has its own node count, and out[s] receives one float64 per node of segment s.  A level
 * buffer of a packet tree is one segment, so a whole tree is one call.  With t over the elements of a node, every term evaluated and
 * accumulated in float64 for both data types:
 *   MIFWT_COST_SHANNON    -sum t^2 ln t^2            (an element whose square is 0 contributes 0)
 *   MIFWT_COST_LOGENERGY  sum ln t^2                 (likewise 0)
 *   MIFWT_COST_NORM       sum |t|^param              (param >= 1 is the caller's; no pow for 1 and 2)
 *   MIFWT_COST_THRESHOLD  #{|t| > param}             (an exact count)
 *   MIFWT_COST_SURE       n - #{|t| <= param} + sum min(t^2, param^2)
 *   mifwt_cost_nodes      kernel id 61, from the node length alone: a node of at most mifwt_cost_short_limit(dtype) elements is summed by
 *                         a group of 4 / 16 / 64 lanes of a workgroup that takes a run of consecutive nodes, and stored at once; a longer
 *                         one is cut into chunks of about mifwt_cost_chunk(dtype) elements, a workgroup and one plain store into
 *                         `workspace` each (8 bytes per unit of mifwt_cost_plan; read only when a segment has long nodes), which a second
 *                         launch (id 62) adds per node in index order.  No atomics; the plan depends on dtype and shapes only, so the
 *                         same input gives the same bits.
 *   mifwt_cost_plan       (host only) the number of units of a table; unit_start, if not NULL, receives nseg + 1 first units.
 * Nothing is copied to the host and nothing synchronises: the call can be captured.  MIFWT_ERR_BADARG for nseg outside
 * [1, mifwt_cost_max_segments()], an unknown dtype or functional, a non-unit innermost stride, a rows_per_index that does not divide the
 * rows, an empty segment or a NULL pointer; MIFWT_ERR_UNSUPPORTED beyond the index range (2^30 elements per row, 2^31 rows, 2^31 elements
 * per node, 2^31 units); MIFWT_ERR_WORKSPACE for a workspace that is too small.  Nothing is launched then.  Not counted by
 * mifwt_launch_count. */
#define MIFWT_KID_COST_NODES 61  /* the costs of the nodes of up to mifwt_cost_max_segments() segments, one launch */
#define MIFWT_KID_COST_FINISH 62 /* the chunks of every long node added in index order */
#define MIFWT_COST_SHANNON 0
#define MIFWT_COST_LOGENERGY 1
#define MIFWT_COST_NORM 2
#define MIFWT_COST_THRESHOLD 3
#define MIFWT_COST_SURE 4
int mifwt_cost_max_segments(void);
int64_t mifwt_cost_short_limit(int dtype);
int64_t mifwt_cost_chunk(int dtype);
int64_t mifwt_cost_plan(int dtype, const mifwt_estim_band* segs, int nseg, int64_t* unit_start);
int mifwt_cost_nodes(int dtype, int functional, double param, const mifwt_estim_band* segs, int nseg, double* const* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* MULTIRESOLUTION ANALYSIS — every component of a decomposition back in the signal domain, all of them in one launch
 * (csrc/mifwt_mra.hip).  MIFWT_F32 / MIFWT_F64, even L <= 20, unit innermost strides.  A COMPONENT is the synthesis of ONE band with
 * every other band absent: `depth` one-input stages, the first with rec_hi (`detail` != 0) or rec_lo, the others with rec_lo.  Band b
 * is [rows, len] at `x` with `row_stride` elements between rows (any view: nothing is copied), and its component is written to
 * out + index * out_comp_stride + row * out_row_stride, n samples per row.  A workgroup takes one (tile of mifwt_mra_tile() outputs,
 * band, row), stages the window of the band its tile depends on into LDS through the boundary's index map, runs the stages between two
 * LDS buffers and writes its tile once.  float32 data is summed in float32 FMAs, float64 in float64; no atomics, nothing is read
 * back: the calls can be captured.
 *   mifwt_mra_swt   kernel id 63, stationary (mifwt_swt_inv with one band absent; len = n).  The stage of level l, l = depth .. 1, has
 *                   dilation D = 2^(l-1):   y[n] = 0.5 sum_i r[i] c[(n + D (L/2 - 1 - i)) mod N]
 *                   so that  D_j = U_1 .. U_{j-1} G_j W_j  and  S_n = U_1 .. U_n V_n  (U: rec_lo, G: rec_hi).  The window a tile needs at
 *                   depth j grows by (2^j - 1) L/2 on the left and (2^j - 1)(L/2 - 1) on the right; it wraps as often as N asks.
 *   mifwt_mra_dwt   kernel id 64, decimated.  level_len[l], l = 0 .. nlevels, is the length of a row at level l (0: the signal, n); a
 *                   band of depth j has level_len[j] samples.  A stage takes level l to l - 1; even / odd outputs use the even / odd
 *                   taps.  Padded (`circular` 0; the synthesis does not depend on the padding mode):
 *                       y[n] = sum_k c[k] r[n + L - 2 - 2k],  n in [0, level_len[l-1]),  level_len[l-1] = 2 level_len[l] - L + 2 or one less
 *                   periodized (`circular` != 0):
 *                       y[(2k + t - L/2 + 1) mod 2 level_len[l]] += c[k] r[t],  level_len[l-1] = 2 level_len[l] or one less
 *                   A level shorter than its full synthesis loses its LAST sample.
 *   mifwt_mra_max_depth  (host only, needs no device) the deepest component the launch of `transform` takes: for MIFWT_MRA_SWT the largest
 *                   j with (2^j - 1)(L - 1) <= 2048 — two LDS buffers of 4096 elements under a 2048-sample tile: db4 to 8, db10 to 6 —,
 *                   for MIFWT_MRA_DWT 32; 0 for 16-bit storage and L > 20.
 * MIFWT_ERR_BADARG for a NULL pointer, an odd L, nbands < 1, a depth < 1, level lengths that are not one decomposition's;
 * MIFWT_ERR_UNSUPPORTED for L > 20, 16-bit storage, more than mifwt_mra_max_bands() bands, a band deeper than mifwt_mra_max_depth, rows
 * or n above 2^30, or (periodized levels of very few samples) a window that outgrows the LDS buffers.  Nothing is launched then.  Not
 * counted by mifwt_launch_count. */
#define MIFWT_KID_MRA_SWT 63 /* all components of a stationary decomposition, one launch */
#define MIFWT_KID_MRA_DWT 64 /* all components of a decimated decomposition (padded or periodized), one launch */
#define MIFWT_MRA_SWT 0
#define MIFWT_MRA_DWT 1
typedef struct mifwt_mra_band {
  const void* x;
  int64_t row_stride; /* elements */
  int32_t index;      /* which component of `out` */
  int32_t depth;      /* stages */
  int32_t detail;     /* first stage: 0 rec_lo, else rec_hi */
  int32_t reserved;
} mifwt_mra_band;
int64_t mifwt_mra_tile(void);
int mifwt_mra_max_bands(void);
int mifwt_mra_max_depth(int dtype, int filt_len, int transform);
int mifwt_mra_swt(int dtype, int filt_len, int64_t rows, int64_t n, const mifwt_mra_band* bands, int nbands, void* out,
                  int64_t out_comp_stride, int64_t out_row_stride, const double* rec_lo, const double* rec_hi, void* stream);
int mifwt_mra_dwt(int dtype, int filt_len, int circular, int64_t rows, const int64_t* level_len, int nlevels, const mifwt_mra_band* bands,
                  int nbands, void* out, int64_t out_comp_stride, int64_t out_row_stride, const double* rec_lo, const double* rec_hi,
                  void* stream);

/* SELECTION — the k-th largest magnitude of a coefficient container, pooled per image (csrc/mifwt_select.hip): what keeps the k largest
 * coefficients of every image when mifwt_thresh_fwd reads it as a threshold.  MIFWT_F32 / MIFWT_F64.  `segs` are bands as above that
 * share `images`; per image all their elements form one multiset of n magnitudes (empty bands are skipped; n < 2^31).
 *   mifwt_select_kth        value[g] = s[n - k], s the ascending sort of |x| of image g: exact, the bits a sort gives, selected on the
 *                           bit pattern with the sign cleared.  k = 0 gives +inf.  k is the argument (0 <= k <= n) or, where dk is not
 *                           NULL, dk[g * dk_stride] (dk_stride 1, or 0: one k for all images), read on the device when the kernel runs
 *                           and clipped to [0, n] there.  value ([images], the data's type) and value64 (the same values as float64,
 *                           what mifwt_thresh_fwd takes as dvalue) may each be NULL.  `route` is MIFWT_KID_SELECT_KTH_LDS (54: one
 *                           workgroup per image, the keys of all segments in LDS; at most mifwt_select_max_segments() non-empty
 *                           segments and mifwt_estim_lds_capacity(dtype) pooled elements per image) or MIFWT_KID_SELECT_KTH_STREAM (55:
 *                           the digit passes of mifwt_estim_stream_plan over all segments with integer counters in `workspace`,
 *                           mifwt_select_workspace bytes, zeroed on the stream; any number of segments, mifwt_select_max_segments()
 *                           per launch, several launches of a pass adding into the same counters).  NaNs are unspecified.
 *   mifwt_select_route      (host only) the default route; 0: nothing to launch (no image or an empty pool).
 * Nothing is copied to the host and nothing synchronises: the calls can be captured.  Integer counters only: the same input gives the
 * same bits.  MIFWT_ERR_BADARG for an unknown dtype or route, a band mifwt_estim_* would refuse, bands of other image counts, k outside
 * [0, n]; MIFWT_ERR_UNSUPPORTED beyond the index range (2^31 pooled elements per image) or, for route 54, its capacity;
 * MIFWT_ERR_WORKSPACE for a workspace that is too small.  These launches are not counted by mifwt_launch_count. */
#define MIFWT_KID_SELECT_KTH_LDS 54    /* k-th largest |x| of a container per image, the image's keys resident in LDS */
#define MIFWT_KID_SELECT_KTH_STREAM 55 /* k-th largest |x| of a container per image, streaming digit passes with integer counters */
int mifwt_select_max_segments(void);
int mifwt_select_route(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int force_stream);
size_t mifwt_select_workspace(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int route);
int mifwt_select_kth(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int64_t k, const int64_t* dk,
                     int64_t dk_stride /* 0: one k for all images */, int route, void* value, double* value64, void* workspace,
                     size_t workspace_bytes, void* stream);

/* COMPACTION — the k kept coefficients of every image of a container as (values, ascending flat indices), and back
 * (csrc/mifwt_compact.hip).  MIFWT_F32 / MIFWT_F64.  `segs` are bands as above that share `images`; the FLAT INDEX of a pooled element is
 * its position in the image's pool: the non-empty segments in order, inside a segment the row-major index of the element within its
 * image.  With key(x) the bit pattern of x with the sign cleared, v = value[g] the k-th largest magnitude of image g
 * (mifwt_select_kth with the same k) and E = k - #{key > key(v)}, the element of flat index i is kept iff
 *         key(x_i) > key(v)   or   ( key(x_i) == key(v)  and  #{ j < i : key(x_j) == key(v) } < E ):
 * every greater element and the first E ties in flat-index order, exactly k elements; with k = 0, none.
 *   mifwt_compact_encode    values[g][j] / indices[g][j], j < counts[g] = k: the kept elements (their original values) and their flat
 *                           indices, ascending; slots counts[g] <= j < capacity hold value 0 and index -1.  k is the argument
 *                           (0 <= k <= capacity) or, where dk is not NULL, dk[g * dk_stride] read on the device and clipped to
 *                           [0, min(n, capacity)] there (the selection must have seen the same clipped k).  0 <= capacity <= n.
 *                           `route` is MIFWT_KID_COMPACT_LDS (56: one workgroup per image, the values of all segments in LDS; the
 *                           limits of route 54) or MIFWT_KID_COMPACT_STREAM (57: count per unit, scan per image, write per unit over a
 *                           unit table in `workspace`, mifwt_compact_workspace bytes; any number of segments,
 *                           mifwt_compact_max_segments() per count / write launch).  NaNs are unspecified.
 *   mifwt_compact_move      (58) scatter (gather = 0): tensors[s][g][i - start_s] = values[g][j] for every j < counts[g] with
 *                           i = indices[g][j] >= 0 inside the pool; gather (gather != 0): the other way.  tensors[s] is dense storage
 *                           [images][sizes[s]], start_s the sum of the sizes before s.  Everything else is left as it is: a scatter
 *                           goes into zero-filled storage, a gather into zero-filled values.  Indices outside [0, n) move nothing.
 *   mifwt_compact_route     (host only) the default encode route; 0: nothing to launch (no image or an empty pool).
 * Nothing is copied to the host and nothing synchronises: the calls can be captured.  No atomics: every output element has one writer,
 * the same input gives the same bits.  Error codes as for mifwt_select_*; MIFWT_ERR_BADARG also for a capacity outside [0, n] and for
 * NULL outputs.  These launches are not counted by mifwt_launch_count. */
#define MIFWT_KID_COMPACT_LDS 56    /* the k kept elements of a container per image, compacted; the image's values resident in LDS */
#define MIFWT_KID_COMPACT_STREAM 57 /* the same, streaming: count per unit, scan per image, write per unit */
#define MIFWT_KID_COMPACT_MOVE 58   /* scatter / gather between compacted (values, indices) and dense per-tensor storage */
int mifwt_compact_max_segments(void);
int mifwt_compact_route(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int force_stream);
size_t mifwt_compact_workspace(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int route);
int mifwt_compact_encode(int dtype, const mifwt_estim_band* segs, int nseg, int64_t images, int64_t k, const int64_t* dk,
                         int64_t dk_stride /* 0: one k for all images */, int64_t capacity, int route, const void* value, void* values,
                         int32_t* indices, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int mifwt_compact_move(int dtype, int gather, void* const* tensors, const int64_t* sizes, int nseg, int64_t images, int64_t capacity,
                       void* values, const int32_t* indices, const int32_t* counts, void* stream);

/* PACKING — a coefficient container as ONE tensor and back (csrc/mifwt_pack.hip): the copies behind coeffs_to_array / ravel_coeffs and the
 * copy=True forms of array_to_coeffs / unravel_coeffs.  Nothing is computed: `elem_bytes` (2, 4, 8 or 16) is the element size, which is
 * all the kernels know of the dtype.  A BOX is a block of four extents, three outer ones and a row, somewhere in the destination:
 *   dst, dst_stride   its first destination element and the element strides of the three outer extents; destination rows are dense
 *   src, src_stride   its first source element and the element strides of all four extents (any: a band is read as the strided view it
 *                     is); src = NULL: the box is filled with the padding element (mifwt_pack_to_array only)
 *   extent            fewer than 2^31 elements per row, fewer than 2^31 rows per box, fewer than 2^31 units per call
 * The caller's boxes must tile what it wants written: every destination element of a box is written once, every source element of a
 * box read once, nothing outside a box is touched.  All offsets are 64-bit.
 *   mifwt_pack_to_array  (59) up to mifwt_pack_max_boxes() boxes in one launch, fills included; `padding`: elem_bytes bytes on the HOST
 *   mifwt_pack_to_bands  (60) the same table run the other way (the array is the source, dense bands the destinations); no fills
 *   mifwt_pack_plan      (host only) the number of units (workgroup iterations) of the call
 *   mifwt_pack_max_tensors  how many tensors of a container the host layer puts into one launch (24, as mifwt_thresh_max_segments);
 *                        mifwt_pack_max_boxes() (40) is what those and the fills between them need in 3-D
 * Nothing is copied to the host and nothing synchronises: the calls can be captured.  MIFWT_ERR_BADARG for another element size, nbox
 * outside [1, mifwt_pack_max_boxes()], a negative extent, a NULL or misaligned pointer of a non-empty box; MIFWT_ERR_UNSUPPORTED
 * beyond the index range.  Nothing is launched then, nor for a call whose boxes are all empty.  Counted under their ids by
 * mifwt_launch_count. */
#define MIFWT_KID_PACK_TO_ARRAY 59 /* the bands of a container and the padding between them into one dense array, one launch */
#define MIFWT_KID_PACK_TO_BANDS 60 /* blocks of one array into dense tensors, one launch */
typedef struct mifwt_pack_box {
  const void* src;
  void* dst;
  int64_t extent[4];
  int64_t src_stride[4];
  int64_t dst_stride[3];
} mifwt_pack_box;
int mifwt_pack_max_boxes(void);
int mifwt_pack_max_tensors(void);
int64_t mifwt_pack_plan(int elem_bytes, const mifwt_pack_box* boxes, int nbox);
int mifwt_pack_to_array(int elem_bytes, const mifwt_pack_box* boxes, int nbox, const void* padding, void* stream);
int mifwt_pack_to_bands(int elem_bytes, const mifwt_pack_box* boxes, int nbox, void* stream);

/* Reduction behind the gradients w.r.t. the FILTER TAPS (learnable wavelets: src/ptwt/wavelets_learnable.py; the reference
 * gets them from ATen's conv backward because its taps stay in the autograd graph, src/ptwt/_util.py:132):
 *     out[t] += sum_{row < rows} sum_{k < m_len} a[row, k] * b_ext[row, 2k + c0 + sgn * t],     t in [0, filt_len)
 * a: rows x m_len, b: rows x n_len (contiguous samples, row strides in elements), b extended by `mode` (enum mifwt_mode);
 * out: DEVICE array of filt_len doubles, accumulated into (zero it first).  f32 / f64.
 *   analysis level,  dL/d dec[m]:  a = upstream gradient of the band, b = level input, c0 = 1,        sgn = -1, mode = level's
 *   synthesis level, dL/d rec[t]:  a = the band,                     b = upstream gradient of y, c0 = -(L-2), sgn = +1, zero mode
 * (for N-D levels a / b are taken after the other axes have been transformed; the host layer composes that). */
int mifwt_tap_correlate(int dtype, int64_t rows, int64_t m_len, int64_t n_len, const void* a, int64_t a_row_stride,
                        const void* b, int64_t b_row_stride, int filt_len, int c0, int sgn, int mode, double* out,
                        void* stream);
/* The same reduction for the STATIONARY levels (mifwt_swt_fwd / mifwt_swt_inv: stride 1, dilation D, periodic with any number of
 * wraps):     out[t] += sum_{row < rows} sum_{k < n} a[row, k] * b[row, (k + c0 + tstep * t) mod n],     t in [0, filt_len)
 *   swt level,  dL/d dec[m]:  a = upstream gradient of the band, b = level input,        c0 = D L/2,       tstep = -D
 *   iswt level, dL/d rec[j]:  a = upstream gradient of y,        b = the band (a or d),  c0 = D (L/2 - 1), tstep = -D  (times the
 *   level's scale, which the host applies).  f32 / f64. */
int mifwt_tap_correlate_dilated(int dtype, int64_t rows, int64_t n, const void* a, int64_t a_row_stride, const void* b,
                                int64_t b_row_stride, int filt_len, int64_t c0, int64_t tstep, double* out, void* stream);

/* Scratch bytes one call needs (0 on the fused paths).  direction: 0 = analysis, 1 = synthesis,
 * 2 = mifwt_dwt_fwd_adjoint, 3 = mifwt_dwt_inv_adjoint (same numbering for mifwt_kernel_id). */
size_t mifwt_workspace_bytes(const mifwt_level_desc* desc, int direction);

/* Which kernel family a call would dispatch to (tests use it to assert the fast path is the one that ran);
 * negative = error code.
 *   0  generic per-axis passes (any strides, any L <= 128; f32 / f64 / f16 / bf16 storage — the fallback of every call no fused kernel takes)
 *   1 / 2  fused single-launch 2-D analysis / synthesis level, streaming wave strips (f32, even L <= 16)
 *   7 / 8  fused single-launch 2-D analysis / synthesis level, LDS tiles (f32 / f16 / bf16, even L <= 20, 24, 32; f64, even L <= 16); the
 *          default 2-D kernels — the streaming analysis kernel is kept for 16-tap filters on planes >= ~1500^2
 *   3 / 4  streaming axis passes, analysis / synthesis: inner-axis kernel (+ one outer-axis pass per further
 *          axis); unit innermost stride, f32 / f64 / f16 / bf16, L in {2..20 even, 24, 32}
 *   5 / 6  3-D analysis / synthesis (f32, even L <= 16; what the brick kernels 9 / 10 do not take): fused 2-D kernel over every
 *          depth slice + one streaming pass along depth
 *   9 / 10  fully fused 3-D analysis / synthesis level, LDS bricks (f32, L in {2, 4, 6}; synthesis also 8): the small volumes
 *   24 / 25  fully fused 3-D analysis / synthesis level, workgroups walking along the depth axis (f32 and f64; analysis: even L <= 10,
 *          every mode, rows <= 512 samples (f64: 256), picked from 2^22 samples per volume on and for 8 taps; synthesis: even L <= 8,
 *          dense coefficient rows, picked from 2^20 output samples on; f64, which has no bricks: analysis from 2^15 / 2^17 / 2^19 samples
 *          on for <= 4 / 6 / 8 taps, synthesis from 2^16 (<= 4 taps) / 2^19 output samples on).  Round 6: batches of 8 / 16 volumes and
 *          more from 2^21 / 10^5 samples per volume on (L <= 6); a SLAB form of the analysis kernel for 8 / 10 taps on rows of at most
 *          128 samples (f32, every mode: a workgroup filters every staged row once), picked by volume and batch (mifwt_dwt3_fwd_slab_plan)
 *   11 / 23  fused 2-D analysis / synthesis level on the matrix cores (banded-Toeplitz MFMA; f16 / bf16 storage, even L in [18, 32]; both walk down
 *          column panels; the synthesis kernel from 16 tiles of 32 x 128 samples per call on, the vector tile kernel 8 below that)
 *   12 / 13  two fused 2-D analysis / synthesis levels per launch (mifwt_dwt2_fwd_pair / mifwt_dwt2_inv_pair; never
 *          returned by mifwt_kernel_id, which describes single-level calls)
 *   14 / 15  the deep levels of a 1-D analysis / the coarse levels of a 1-D synthesis in one launch (mifwt_dwt1_fwd_tail /
 *          mifwt_dwt1_inv_tail; likewise not returned by mifwt_kernel_id)
 *   16     up to three fused 2-D analysis levels per launch (mifwt_dwt2_fwd_pyramid; not returned by mifwt_kernel_id)
 *   17 / 18  several fused 1-D analysis / synthesis levels of long rows, a chunk per workgroup (mifwt_dwt1_fwd_long /
 *          mifwt_dwt1_inv_long; likewise)
 *   20 / 21  every level of a 2-D analysis / synthesis of a small plane in one launch (mifwt_dwt2_fwd_pyramid's second kernel /
 *          mifwt_dwt2_inv_pyramid; likewise)
 *   22     up to three fused 2-D synthesis levels of a big plane per launch (mifwt_dwt2_inv_pyramid's second kernel; likewise)
 *   26 / 27  fused boundary-wavelet analysis / synthesis level, 1-D and 2-D (mifwt_bwt_fwd / mifwt_bwt_inv; answered by mifwt_bwt_kernel_id)
 *   28 / 29  one axis of a boundary-wavelet level through a run-time tap loop (mifwt_bwt_axis_fwd / mifwt_bwt_axis_inv)
 *   30 / 31  fused 3-D boundary-wavelet analysis / synthesis level, LDS bricks (mifwt_bwt3_fwd / mifwt_bwt3_inv; f32 / f64, even L <= 8;
 *          answered by mifwt_bwt3_kernel_id)
 *   32 / 33  a subtree (two or more levels) of a 1-D boundary-wavelet packet tree per launch, analysis / synthesis, one row per workgroup
 *          (mifwt_bwt_tree_fwd / mifwt_bwt_tree_inv; f32 / f64, even L <= 20; answered by mifwt_bwt_tree_levels)
 *   38 / 39  fused periodized analysis / synthesis level, 1-D and 2-D (mifwt_per_fwd / mifwt_per_inv; answered by mifwt_per_kernel_id)
 *   40 / 41  one axis of a periodized level through a run-time tap loop (mifwt_per_axis_fwd / mifwt_per_axis_inv)
 *   42 / 43  fused value-map extension analysis level / its adjoint, 1-D and 2-D (mifwt_ext_fwd / mifwt_ext_adj; answered by mifwt_ext_kernel_id)
 *   44 / 45  one axis of such a level / of its adjoint through a run-time tap loop (mifwt_ext_axis_fwd / mifwt_ext_axis_adj)
 *   46 / 47  fused analysis / padded synthesis level of interleaved complex data, 1-D and 2-D (mifwt_cplx_fwd / mifwt_cplx_inv; answered by
 *          mifwt_cplx_kernel_id; counted under their ids by mifwt_launch_count)
 *   48 / 49  thresholding of up to mifwt_thresh_max_segments() tensors per launch / its backward (mifwt_thresh_fwd / mifwt_thresh_bwd;
 *          never returned by mifwt_kernel_id; counted under their ids by mifwt_launch_count)
 *   50 / 51  exact order statistics of |x| per leading index: an image's keys in LDS / streaming digit passes (mifwt_estim_sigma;
 *          answered by mifwt_estim_select_route)
 *   52 / 53  sums of x^2 of a container's bands + BayesShrink thresholds / VisuShrink thresholds (mifwt_estim_thresholds)
 *   54 / 55  the k-th largest |x| of a container pooled per leading index: the keys in LDS / streaming digit passes (mifwt_select_kth;
 *          answered by mifwt_select_route)
 *   56 / 57  the k kept elements of a container per leading index as (values, ascending flat indices): the values in LDS / streaming
 *          count, scan and write (mifwt_compact_encode; answered by mifwt_compact_route)
 *   58     scatter / gather between compacted (values, indices) and dense per-tensor storage (mifwt_compact_move)
 *   59 / 60  the tensors of a container and the padding between them into one dense array / blocks of one array into dense tensors,
 *          a box table per launch (mifwt_pack_to_array / mifwt_pack_to_bands; never returned by mifwt_kernel_id)
 *   61 / 62  the additive costs of the nodes of a packet tree, every level a segment of one launch / the chunks of the long nodes added
 *          in order (mifwt_cost_nodes; never returned by mifwt_kernel_id)
 *   63 / 64  every component of a multiresolution analysis in one launch: stationary / decimated (mifwt_mra_swt / mifwt_mra_dwt;
 *          never returned by mifwt_kernel_id) */
int mifwt_kernel_id(const mifwt_level_desc* desc, int direction);

/* Library-wide diagnostic switches (process-global, meant for tests and A/B measurements).
 *   MIFWT_OPT_FORCE_GENERIC (0): non-zero routes every call through the generic per-axis passes.
 *   MIFWT_OPT_ROWS_PER_CHUNK (1): >0 overrides the fused kernels' output rows per streamed chunk.
 *   MIFWT_OPT_PREFETCH_PAIRS (2): >0 overrides the fused kernels' register-ring prefetch depth. */
#define MIFWT_OPT_FORCE_GENERIC 0
#define MIFWT_OPT_ROWS_PER_CHUNK 1
#define MIFWT_OPT_PREFETCH_PAIRS 2 /* >0 overrides the fused kernels' prefetch depth (row pairs in flight) */
#define MIFWT_OPT_RESERVED3 3      /* unused (was: cooperative full-line writer, removed after measurement) */
#define MIFWT_OPT_NT_STORE 4       /* non-zero: nontemporal stores for the sub-band planes */
#define MIFWT_OPT_TILE_MODE 5      /* 2-D analysis: 0 = auto (LDS-tile kernel on small planes), 1 = always tile, 2 = never.  3-D: 0 = auto (depth-walking kernels 24 / 25 on big volumes, bricks 9 / 10 on small ones), 1 = bricks wherever they can run, 2 = composed route, 4 = walking kernels wherever they can run */
#define MIFWT_OPT_TILE_ROWS 6      /* >0 overrides the tile kernels' output rows per tile */
#define MIFWT_OPT_MFMA_MODE 7      /* 2-D analysis, f16 / bf16 storage, 18..32 taps: 0 = matrix-core kernels (walking down column panels), 2 = vector tile
                                      kernels, 3 = the tile-at-a-time analysis kernel of round 2 (comparisons), 4 = the synthesis kernel for every size */
#define MIFWT_OPT_PAIR_MODE 8      /* multi-level launches (mifwt_dwt2_fwd_pyramid, mifwt_dwt2_fwd_pair, mifwt_dwt2_inv_pair, mifwt_dwt1_fwd_tail): 2 = never (they answer
                                      UNSUPPORTED / 0); analysis pairs: 0 = auto (rolling strips for 8 taps, else tiles), 1 = tiles only,
                                      3 = rolling strips wherever they apply */
#define MIFWT_OPT_PAIR_ROWS 9      /* >0 overrides the pair kernels' level-2 rows per tile (4, 6, 8, 12) / per strip segment (multiple of 8) */
#define MIFWT_OPT_PYRAMID_MODE 12 /* mifwt_dwt2_fwd_pyramid: 0 = auto (each of its two kernels where it is the fastest route), 1 = the streaming kernel wherever it can run, 3 = the small-plane kernel wherever it can run, 2 = never (it answers UNSUPPORTED / 0; the two-level and per-level kernels then serve the call) */
#define MIFWT_OPT_DEBUG 11        /* ROUTING bits: alternative code paths with the SAME results (A/B runs, parity tests): 8 = the streaming synthesis kernel (id 22) without its fast warm-up, 64 = column strips of 64 instead of balanced strips (3-D analysis walk), 512 = 8-byte instead of 16-byte output stores (3-D synthesis walk), 1024 = analysis adjoints with a boundary extension on the generic per-axis passes instead of synthesis launch + border kernel, 4096 = the border part of a 2-D analysis adjoint on the one-thread-per-sample kernel instead of the one-thread-per-border-line kernel, 8192 = the level-2 waves of the streaming analysis kernel (id 16) behind the step's second barrier, 1 << 19 = kernel 16 without its tail wave, 1 << 20 = kernel 16 in its sixteen-wave form.  Any other bit is a MEASUREMENT switch that breaks results (no stores / no loads / no deep levels / single passes off ...): those are compiled into -DMIFWT_DIAG builds only (tools/; csrc/mifwt_common.h) and the product library answers MIFWT_ERR_UNSUPPORTED to them */
#define MIFWT_OPT_PYR_WGS 13 /* >0: the streaming analysis kernel (id 16) cuts the batch's rows into this many chunks (workgroups per column group) instead of one per CU — parity tests of units that start and end anywhere */
#define MIFWT_OPT_EXP 15           /* experiment word of the A/B run in progress (tools/): -DMIFWT_DIAG builds only; the product library accepts 0 and answers MIFWT_ERR_UNSUPPORTED to anything else */
#define MIFWT_OPT_SYNC_STAGE 10    /* non-zero: tile kernels keep the workgroup barrier between staging and the horizontal pass (A/B) */
int mifwt_set_option(int key, int value);

/* Diagnostic (-DMIFWT_DIAG builds; the product library has no profiling instances and answers MIFWT_ERR_UNSUPPORTED to a non-null
 * buffer): a device buffer of 2 x uint64 per wave of every workgroup that later mifwt_dwt2_fwd_pyramid launches fill with
 * (cycles alive, cycles spent in workgroup barriers); NULL switches it off again. */
int mifwt_pyr_profile_buffer(void* device_buffer);

/* Diagnostic: how many launches of a kernel VARIANT this process has enqueued — variants that share a kernel id (what the tests use to
 * pin "this code path ran"; `variant` out of range: 0).  Values below 16 are variants; the 2-D and 3-D stationary kernels and the
 * periodized and value-map extension kernels (MIFWT_KID_PER_*, MIFWT_KID_EXT_*, 38 .. 45), which have no variants, are counted under
 * their kernel ids. */
#define MIFWT_VARIANT_FWD_MFMA_WALK 0 /* id 11: the analysis kernel that walks down column panels */
#define MIFWT_VARIANT_FWD_MFMA_TILE 1 /* id 11: the tile-at-a-time analysis kernel of round 2 (MIFWT_OPT_MFMA_MODE 3) */
#define MIFWT_VARIANT_FWD_PYR_ST16 2  /* id 16: 16-byte stores after a lane-pair exchange (planes with 16-byte aligned rows) */
#define MIFWT_VARIANT_FWD_PYR_ST8 3   /* id 16: 8-byte stores (any row pitch) */
#define MIFWT_KERNEL_SWT2_FWD 34       /* id 34: fused 2-D stationary analysis level (mifwt_swt2_fwd) */
#define MIFWT_KERNEL_SWT2_INV 35       /* id 35: fused 2-D stationary synthesis level (mifwt_swt2_inv) */
#define MIFWT_KERNEL_SWT3_FWD 36       /* id 36: fused 3-D stationary analysis level (mifwt_swt3_fwd) */
#define MIFWT_KERNEL_SWT3_INV 37       /* id 37: fused 3-D stationary synthesis level (mifwt_swt3_inv) */
#define MIFWT_VARIANT_TAPCORR_ROWS 50   /* tap-gradient correlation along contiguous rows: a wave per (row, 64-coefficient chunk) task */
#define MIFWT_VARIANT_TAPCORR_COLS 51   /* ... along the rows of planes: a wave per (image, row chunk, 64-column strip) task */
#define MIFWT_VARIANT_TAPCORR_TERM 52   /* ... one thread per term in a 64-bit loop: dilated, long, or more than 2^31 wave tasks */
#define MIFWT_LAUNCH_COUNTERS 64
unsigned long long mifwt_launch_count(int variant);

const char* mifwt_strerror(int code);
int mifwt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MIFWT_H */
