/*
 * dvae_hip.h — C ABI of libdvae_hip.so: the MI355X (gfx950) kernels behind the
 * disentangled-VAE training step.
 *
 * The reference (v-manhlt3/Disentangle-VAE-for-VC) has no FFI/plugin layer: its
 * hot path reaches ATen/cuDNN through torch.nn.  Each entry point below names
 * the reference construct (file:line under /root/reference) whose tensor math it
 * replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (workspaces too);
 *     the library allocates nothing and keeps no state between calls, except
 *     the opt-in profiling event pool (dvae_prof_*);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *     no call synchronises the device;
 *   - return value: 0 on success, a negative DVAE_E* code otherwise; nothing
 *     throws, nothing exits;
 *   - activations are FRAME-MAJOR: a tensor "[T, N, C]" holds frame t of mel
 *     segment n at row r = t*N + n of a row-major [T*N, C] matrix.  N counts
 *     segments of the utterance PAIR batched together (x1 rows first, then x2),
 *     so BatchNorm statistics are taken per GROUP of N/G consecutive segments.
 *   - all arithmetic is fp32 (MFMA v_mfma_f32_32x32x2_f32 / 16x16x4_f32).
 */
#ifndef DVAE_HIP_H
#define DVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_OK 0
#define DVAE_EINVAL (-1)  /* bad shape / alignment / null pointer */
#define DVAE_ELAUNCH (-2) /* hipLaunch failed; see dvae_last_hip_error() */

#define DVAE_ACT_NONE 0
#define DVAE_ACT_RELU 1
#define DVAE_ACT_TANH 2

#define DVAE_EPI_STORE 0  /* C  = result                    */
#define DVAE_EPI_ACCUM 1  /* C += result (plain read-modify-write, no split-K) */
#define DVAE_EPI_ATOMIC 2 /* C += result with global_atomic_add_f32 (split-K allowed) */

/* ABI revision of this header; dvae_version() of the loaded library must return exactly this (the ctypes binding
 * refuses anything else: a stale .so would misread the argument lists below).  The latent report's two entry points
 * (dvae_latent_tables, dvae_latent_lse) were added at 319 without a new revision: the change is purely additive, no
 * existing argument list, structure or constant moved.  Likewise the scheduled loss (dvae_loss_fwd_sched,
 * dvae_loss_bwd_sched, dvae_loss_sched_t, DVAE_LOSS_MAX_D): additive, and the suites of the two earlier additions pin 319.
 * Likewise the latent map's four entry points (dvae_tsne_nn, dvae_tsne_affinities, dvae_tsne_forces, dvae_tsne_update) and
 * the speaker adversary's two (dvae_adv_rows, dvae_adv_params), and the factor penalty's three (dvae_factor_ws_bytes,
 * dvae_factor_fwd, dvae_factor_bwd), and the modulation-spectrum loss's three (dvae_msloss_ws_bytes, dvae_msloss_fwd,
 * dvae_msloss_bwd). */
#define DVAE_ABI_VERSION 319
int dvae_version(void);

/* ---- arithmetic of a contraction (every GEMM / conv / LSTM entry point takes a `mode` argument):
 * DVAE_MODE_F32    fp32 operands on v_mfma_f32_32x32x2_f32 / 16x16x4_f32 (the fp32 matrix pipe runs at the vector
 *                  rate, 157 TFLOP/s);
 * DVAE_MODE_F32X3  fp32 RESULTS on the bf16 matrix pipe: each fp32 operand is split exactly into three bf16 terms
 *                  (x = x1 + x2 + x3) and a product is the sum of the six partial products whose weight is >= 2^-16,
 *                  each exact in fp32, accumulated in fp32 — the dropped terms are below the rounding of one fp32 FMA,
 *                  so this IS an fp32 contraction (same error against fp64 as DVAE_MODE_F32, tests/test_hip_x3.py) at
 *                  6/16 of its MFMA cost — BASELINE configs[1], [3];
 * DVAE_MODE_BF16   bf16 operands (rounded to nearest-even on their way into the matrix cores) with fp32 accumulation on
 *                  v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16 — BASELINE configs[2], [4] ("bf16 compute");
 * DVAE_MODE_DEFAULT  whatever dvae_set_compute_mode() last set (process-wide default, initially DVAE_MODE_F32).
 * Everything that is not a contraction (BatchNorm, gates, losses, Adam, master weights) is fp32 in every mode. */
/* bf16 mode only, OR-ed into `mode`: the operand / the result is bf16 IN MEMORY (written so by its producer), not fp32
 * rounded on the way into the matrix cores.  A = first operand (activations), B = second (weights), C = result (plain
 * store epilogue only).  Leading dimensions stay in elements; a bf16 operand needs them (and its contiguous extent)
 * to be multiples of 8. */
#define DVAE_MODE_A_BF16 0x100
#define DVAE_MODE_B_BF16 0x200
#define DVAE_MODE_C_BF16 0x400
#define DVAE_MODE_DEFAULT (-1)
#define DVAE_MODE_F32 0
#define DVAE_MODE_BF16 1
#define DVAE_MODE_F32X3 2
int dvae_set_compute_mode(int mode);
int dvae_get_compute_mode(void);

/* Deterministic mode (a TEST mode; off by default, not on the benchmarked path).  The fast path accumulates split-k
 * partial products, column sums and the recurrences' bias gradients with float atomics, whose order — hence the last
 * bits of every gradient — changes from run to run.  With the mode on every accumulated output element has ONE writer
 * in a fixed order: contractions run unsplit (split_k is forced to 1), dvae_colsum_add walks all rows in one
 * workgroup per column block; callers keep the recurrences' bias gradients out of the persistent launches (ops.py).
 * Two runs of the same step on the same inputs are then bit-identical (tests/test_hip_determinism.py). */
int dvae_set_deterministic(int on);
int dvae_get_deterministic(void);
/* hipError_t of the last failed launch (0 if none) */
int dvae_last_hip_error(void);

/* ---- dense contraction (replaces aten::addmm / mm / convolution[_backward]) ----
 * C[M,N] (+)= act( opA(A)[M,K] * opB(B)[K,N] + bias[N] )
 *   a_kcontig = 1: A stored [M][K] (lda = row stride)   0: stored [K][M]
 *   b_kcontig = 1: B stored [N][K] (torch Linear/LSTM weight layout)   0: stored [K][N]
 * lda, ldb must be multiples of 4 and A, B 16-byte aligned; K % 4 == 0 if an operand is k-contiguous,
 * M % 4 == 0 (N % 4 == 0) if A (B) is not.  A, B, C are fp32 unless `mode` carries DVAE_MODE_A/B/C_BF16 (bf16 mode).
 * Replaces: nn.Linear forward/backward (disentangled_vae.py:165-171,194,211-213,232-233,247),
 * LSTM input projections and weight gradients (:163,172,193).
 */
int dvae_gemm_f32(const void* A, const void* B, void* C, const float* bias,
                  int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                  int a_kcontig, int b_kcontig, int act, int epi, int split_k, int mode, void* stream);

/* `batch` (1..4) products of ONE shape in one launch: product b is C[b] (+)= opA(A[b]) * opB(B[b]) (no bias, no
 * activation; epi / split_k / mode as above, storage flags apply to every product).  For contractions too small to fill
 * the chip on their own — the weight gradients of the two directions of the H = 64 encoder BiLSTM (disentangled_vae.py:163):
 * dW_ih, dW_hh of the forward and the reverse direction are two launches of batch 2 instead of four under-filled ones.
 * A, B, C: host arrays of `batch` device pointers (read during the call only), each 16-byte aligned. */
int dvae_gemm_f32_batched(const void* const* A, const void* const* B, void* const* C, int batch, int M, int N, int K,
                          int64_t lda, int64_t ldb, int64_t ldc, int a_kcontig, int b_kcontig, int epi, int split_k,
                          int mode, void* stream);
/* ---- k-split WITHOUT atomics (round 6; replaces the split-K atomic accumulation of every aten::mm / convolution_backward
 * the reference runs through cuBLAS / cuDNN: /root/reference/model/variational_base_vae.py:68 `loss.backward()`) ----
 * A product cut along k stores its partial results PLAINLY: when the launch is split (return value n > 1) EVERY split ks
 * stores into slab + ks * slab_stride (elements; a multiple of 4, >= the extent of C; the slabs 16-byte aligned; conv weight
 * gradients keep their five per-tap outputs at the same distances inside a slab) and C is NOT written; an unsplit launch
 * (n == 1) writes C as `epi` says (DVAE_EPI_STORE / DVAE_EPI_ACCUM).  `slab_cap` = slabs the caller provides: the dispatch may
 * take fewer k-splits than `split_k` asks for, or — the tiles that want one workgroup per CU — more, never more than
 * slab_cap.  RETURNS the number of k-splits launched (>= 1), or a negative error code.  The caller then combines the n
 * slabs in the fixed order ks = 0, 1, ... (dvae_slab_sum now, or dvae_slab_fold later, e.g. at the end of the backward pass):
 * every output element has ONE writer per buffer and ONE summation order, so results are run-to-run bit-identical, and every
 * epilogue is plain 16-byte stores (no read-modify-write, no atomics).  The bias rides split 0; no activation when split
 * (dvae_slab_sum applies it).  dvae_conv5_fwd_slabs / dvae_conv5_dgrad_t_slabs: the convs with <= 128 output columns, which
 * the default arithmetic cuts along k to fill the chip (they return 1 when they did not split). */
int dvae_gemm_f32_slabs(const void* A, const void* B, void* C, float* slab, int64_t slab_stride, int slab_cap,
                        const float* bias, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                        int a_kcontig, int b_kcontig, int epi, int split_k, int mode, void* stream);
/* batched form (dvae_gemm_f32_batched): product b stores split ks into slab (b * n + ks), n = the return value (> 1) */
int dvae_gemm_f32_batched_slabs(const void* const* A, const void* const* B, void* const* C, int batch, float* slab,
                                int64_t slab_stride, int slab_cap, int M, int N, int K, int64_t lda, int64_t ldb,
                                int64_t ldc, int a_kcontig, int b_kcontig, int epi, int split_k, int mode, void* stream);
int dvae_conv5_fwd_slabs(const void* X, const void* Wp, const float* bias, float* Y, float* slab, int64_t slab_stride,
                         int slab_cap, int R, int N, int Cin, int Cout, int mode, void* stream);
int dvae_conv5_dgrad_t_slabs(const void* dY, const void* Wpt, float* dX, float* slab, int64_t slab_stride, int slab_cap,
                             int R, int N, int Cin, int Cout, int mode, void* stream);
int dvae_conv5_wgrad_slabs(const void* dY, const void* X, float* dWp, float* slab, int64_t slab_stride, int slab_cap,
                           int R, int N, int Cin, int Cout, int epi, int split_k, int mode, void* stream);
/* C[i] = act((accumulate ? C[i] : 0) + sum_{k < nslab} slab[k * slab_stride + i]), i < n  (n, slab_stride multiples of 4) */
int dvae_slab_sum(float* C, const float* slab, int64_t slab_stride, int nslab, int64_t n, int act, int accumulate,
                  void* stream);
/* c[i] += sum_{k < nslab} slab[...] for many results in ONE launch per DVAE_SLAB_FOLD_MAX entries (`descs`: read during the call) */
typedef struct {
  float* c;
  const float* slab;
  int64_t slab_stride;
  int64_t n;
  int nslab;
  int pad_;
} dvae_slab_desc_t;
#define DVAE_SLAB_FOLD_MAX 64
int dvae_slab_fold(const dvae_slab_desc_t* descs, int n_entries, void* stream);
/* ---- Conv1d(k=5, stride 1, pad 2) on frame-major data (disentangled_vae.py:111-114, 178-181) ----
 * Weights are used in PACKED form Wp[5][Cout][Cin] (see dvae_conv_pack_w).
 * fwd : Y[R,Cout]   = sum_tap X[r+(tap-2)*N, :] * Wp[tap]^T + bias      (rows outside [0,R) are zero)
 * dgrad: dX[R,Cin]  = sum_tap dY[r-(tap-2)*N, :] * Wp[tap]                  (dvae_conv5_dgrad_t, on the transposed pack)
 * wgrad: dWp[tap][Cout][Cin] += sum_r dY[r, co] * X[r+(tap-2)*N, ci]     (atomic accumulation)
 * R = T*N rows, N = segments per frame.
 */
int dvae_conv5_fwd(const void* X, const void* Wp, const float* bias, float* Y,
                   int R, int N, int Cin, int Cout, int mode, void* stream);
/* conv forward that also leaves the per-column partial sums of Y that a training-mode BatchNorm over G statistics groups
 * needs in bn_ws (>= dvae_bn_ws_bytes(R, Cout, G) bytes): follow with dvae_bn_stats_finalize instead of
 * dvae_bn_stats_fwd — one pass over Y less per block (disentangled_vae.py:151-162: conv -> BatchNorm -> ReLU) */
int dvae_conv5_fwd_stats(const void* X, const void* Wp, const float* bias, float* Y,
                         int R, int N, int Cin, int Cout, int mode, int G, void* bn_ws, void* stream);
int dvae_conv5_wgrad(const void* dY, const void* X, float* dWp,
                     int R, int N, int Cin, int Cout, int split_k, int mode, void* stream);
/* W[Cout][Cin][5] (torch layout, state_dict contract) -> Wp[5][Cout][Cin] */
int dvae_conv_pack_w(const float* W, float* Wp, int Cout, int Cin, void* stream);
/* Wpt[5][Cin][Cout]: the transposed pack; with it the data gradient reads BOTH operands k-contiguously (the faster
 * ds_read_b128 fragment path of the contraction kernel). */
int dvae_conv_pack_wt(const float* W, float* Wpt, int Cout, int Cin, void* stream);
int dvae_conv5_dgrad_t(const void* dY, const void* Wpt, float* dX, int R, int N, int Cin, int Cout, int mode,
                       void* stream);
/* dW[Cout][Cin][5] += dWp[5][Cout][Cin] */
int dvae_conv_unpack_add_w(const float* dWp, float* dW, int Cout, int Cin, void* stream);

/* ---- BatchNorm1d in training mode + activation (disentangled_vae.py:58,69,78,159,182,189; F.relu :202,243; tanh :83) ----
 * Statistics are per GROUP g = (r % N) / (N/G) (one group per encode()/decode()/postnet() call of the
 * reference, which sees x1 and x2 separately).  ws: >= dvae_bn_ws_bytes(R, C, G) bytes.
 * dvae_bn_stats_fwd: mean[G][C], rstd[G][C] (biased var, eps); running_mean/var updated once per group in
 *   group order with `momentum` and the unbiased variance; *num_batches_tracked += G. running_* may be null.
 * dvae_bn_apply_fwd: Z = act((Y-mean)*rstd*gamma + beta) (+ residual if non-null)
 * dvae_bn_bwd: given dZ, saved Y and Z: dY (may alias dZ), dgamma += , dbeta += ; the residual branch's
 *   gradient is dZ itself (handled by the caller).  dY == dZ is allowed with an fp32 dY only: a bf16 dY (dtypes bit 1)
 *   written over the fp32 dZ would overwrite quads that other threads have yet to read, so dvae_bn_bwd and
 *   dvae_bn_bwd_from_y return DVAE_EINVAL for it and write nothing.  dgamma / dbeta may be null (not accumulated).
 */
int64_t dvae_bn_ws_bytes(int R, int C, int G);
int dvae_bn_stats_fwd(const float* Y, float* mean, float* rstd, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, void* ws, int R, int N, int C, int G,
                      float eps, float momentum, void* stream);
/* finalize only: the partial sums are already in ws (left there by dvae_conv5_fwd_stats) */
int dvae_bn_stats_finalize(float* mean, float* rstd, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, const void* ws, int R, int N, int C, int G,
                           float eps, float momentum, void* stream);
int dvae_bn_apply_fwd(const float* Y, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, const float* residual, void* Z,
                      int R, int N, int C, int G, int act, int z_bf16, void* stream);
/* dtypes: bit 0 = Z is bf16, bit 1 = dY is written as bf16 (bf16 compute mode: Z and dY are contraction operands, their
 * producers write them in the storage the consumers read; z_bf16 of dvae_bn_apply_fwd likewise) */
int dvae_bn_bwd(const float* dZ, const float* Y, const void* Z, const float* mean, const float* rstd,
                const float* gamma, void* dY, float* dgamma, float* dbeta, void* ws,
                int R, int N, int C, int G, int act, int dtypes, void* stream);
/* the same without reading Z, for act = ReLU or none: the activation's derivative is recomputed from Y with the forward
 * pass's expression (act((Y-mean)*rstd*gamma + beta) > 0) — 20 instead of 28 bytes per element over the two passes.
 * (tanh blocks keep dvae_bn_bwd: recomputing tanh costs these HBM-bound passes more than the bytes it saves.) */
int dvae_bn_bwd_from_y(const float* dZ, const float* Y, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, void* dY, float* dgamma, float* dbeta, void* ws,
                       int R, int N, int C, int G, int act, int dtypes, void* stream);

/* ---- LSTM recurrence, frame-major, one launch per frame (nn.LSTM at disentangled_vae.py:163,172,193) ----
 * One dvae_lstm_dir_t per direction (1 or 2).  Gate order i,f,g,o (torch).
 * fwd : gates[T,N,4H] holds X*W_ih^T + b_ih + b_hh on entry and the ACTIVATED gates on exit;
 *       h_out[t] (row stride ldh; direction d writes columns [d*H,(d+1)*H) via its own pointer), c_all[T,N,H].
 * bwd : w_hh_t is W_hh transposed, [H][4H]; dh_out = gradient w.r.t. h_out (same strides);
 *       dgates[T,N,4H] = gradient w.r.t. the pre-activation gates; dc_ws[N,H] scratch.
 */
typedef struct {
  float* gates;       /* [T,N,4H] */
  const float* w_hh;  /* fwd: [4H,H]   bwd: W_hh^T [H,4H] */
  float* h_out;       /* fwd: out [T,N,ldh]   bwd: unused */
  float* c_all;       /* [T,N,H] */
  const float* dh_out;/* bwd only: [T,N,ldh] */
  float* dgates;      /* bwd only: [T,N,4H] */
  float* dc_ws;       /* bwd only: [N,H] */
  const float* w_packed; /* optional: weights re-packed in MFMA fragment order by dvae_lstm_pack_w (fwd: packed_fwd,
                            bwd: packed_bwd); when given, the faster 1-KiB-burst frame kernels are used */
  int reverse;        /* 0: t = 0..T-1, 1: t = T-1..0 */
  int packed_mode;    /* DVAE_MODE_F32: w_packed from dvae_lstm_pack_w (fp32 MFMA recurrence); DVAE_MODE_BF16: from
                         dvae_lstm_pack_w_bf16 (bf16 operands / fp32 accumulation on v_mfma_f32_16x16x32_bf16);
                         DVAE_MODE_F32X3: from dvae_lstm_pack_w_x3 (fp32 results: three bf16 planes of W_hh, h split the
                         same way, six exact partial products).  The last two need H % 512 == 0, or H == 64: the whole-sequence
                         kernels of H = 64 take w_hh itself (no w_packed) and round / split it in registers */
  int step_shift;     /* *_range calls: this entry runs its step s in the launch of global step s + step_shift (0 for
                         the plain calls).  Lets two STACKED layers share launches, the upper one a chunk of frames
                         behind the lower one (whose chunk of outputs has meanwhile gone through the upper layer's input
                         projection): twice the workgroups per launch, half the launches */
  int state_bf16;     /* bf16 mode only: h_out (forward call) / dgates (backward call) are bf16 tensors — the storage their
                         consumers (the next frame, the next layer's projection, the weight gradients) read; the same
                         element strides */
  void* pers_ws;      /* optional: >= dvae_lstm_pers_ws_bytes(N, H) bytes, 256-byte aligned, zero-initialised ONCE by the
                         caller and never written by it afterwards: the flags in it count frames across ALL launches (each
                         launch reads the epoch the previous one left, ABI 306: no clearing launch in front of a persistent
                         launch), so a workspace must not be cleared, copied or shared between devices.  When given to a plain one-direction dvae_lstm_seq_fwd / _bwd call whose shape has a
                         persistent kernel (dvae_lstm_pers_supported), the whole sequence
                         runs in ONE W_hh-resident launch (csrc/lstm_pers.hip) instead of one launch per frame; same
                         arithmetic, same tensors.  One workspace serves every layer run on one stream */
  unsigned pers_timeout_us; /* bound of every cross-workgroup wait of that launch (0: 2 s); see dvae_lstm_pers_check */
  float* dbias_ih;    /* optional, used by the PERSISTENT backward launch only (dvae_lstm_pers_supported(.., bwd = 1)): the */
  float* dbias_hh;    /* column sums of dgates over all frames and rows are ADDED to these [4H] vectors (the gradients of
                         b_ih and b_hh, nn.LSTM keeps two): the caller then skips its dvae_colsum_add pass over dgates.
                         Ignored (and the caller must run dvae_colsum_add) when the per-frame kernels are used */
  float* dbias_part;  /* optional, PERSISTENT backward launch only, instead of dbias_ih / dbias_hh (ABI 307): row group rb of the
                         launch STORES its share of the column sums of dgates at dbias_part[(rb * 4 + g) * H + unit] — a
                         [DVAE_PERS_BIAS_SLABS][4H] buffer (row groups the launch does not have are written as zeros) that
                         the caller adds up in the fixed order rb = 0, 1, ... (dvae_slab_sum / dvae_slab_fold with
                         slab_stride 4H): no atomics, run-to-run bit-identical bias gradients */
  int64_t gate_ld;    /* row stride, in elements, of gates and dgates (0: 4H, the dense layout).  H = 64 only: the two
                         directions of the encoder BiLSTM keep their gates side by side in ONE [T*N, 8H] tensor, so that both
                         input projections are one contraction with N = 8H (and both data gradients one with K = 8H);
                         every direction of a call must name the same stride */
} dvae_lstm_dir_t;
#define DVAE_PERS_BIAS_SLABS 16  /* rows of dvae_lstm_dir_t.dbias_part */
/* W_hh [4H,H] -> fragment-ordered copies (each 4H*H floats) for the forward / backward frame kernels.  All three pack
 * entry points move 16-byte vectors: w_hh and every pack given must be 16-byte aligned (DVAE_EINVAL otherwise). */
int dvae_lstm_pack_w(const float* w_hh, float* packed_fwd, float* packed_bwd, int H, void* stream);
/* bf16 compute mode: the same copies rounded to bf16 (each 4H*H bf16 values = 2*4H*H bytes) */
int dvae_lstm_pack_w_bf16(const float* w_hh, void* packed_fwd, void* packed_bwd, int H, void* stream);
/* fp32x3 mode: three bf16 planes per fragment, [..][kc][plane][lane][8] with w1 = rne(w), w2 = rne(w - w1),
 * w3 = w - w1 - w2, so w == w1 + w2 + w3 exactly (each copy 3 * 4H*H bf16 values = 6*4H*H bytes).  "Exactly" holds for
 * 2^-110 <= |w| (and 0): the last bit of w3 lies 23 binary places below w's exponent, and bf16 ends at 2^-133.
 * Below that it does NOT hold in general.  Nothing is flushed: on the MI355X the pack of fp32 SUBNORMAL weights is bit for
 * bit the IEEE split (tests/test_hip_repack.py::test_x3_pack_of_subnormal_weights_is_finite prints it) — w1 = rne(w) on
 * bf16's subnormal grid (multiples of 2^-133), w2 = w3 = 0 (the residual is at most half a step of that grid and rounds to
 * zero), so the planes sum to rne(w), which equals w only for the 1 in 65 536 weights that lie on the grid.  Every plane
 * stays finite. */
int dvae_lstm_pack_w_x3(const float* w_hh, void* packed_fwd, void* packed_bwd, int H, void* stream);
/* ---- all weight-derived operand layouts of a model in ONE launch (once per training step, after Adam) ----
 * kind CONV_T    src Wp[5][d0=Cout][d1=Cin]                 -> dst Wpt[5][Cin][Cout]  (operand of dvae_conv5_dgrad_t)
 *      LSTM_PACK src W_hh[4*d0][d0], d0 = H                 -> dst packed_fwd in mode d1, dst2 packed_bwd in mode d2
 *                                                              (either pointer may be null; DVAE_MODE_F32 / _BF16 /
 *                                                              _F32X3, the last two only where H % 512 == 0): see
 *                                                              dvae_lstm_pack_w / _bf16 / _x3
 *      TRANSPOSE src W[d0][d1]                              -> dst W^T[d1][d0]         (bf16 destination when d2 & 1;
 *                                                                                       CONV_T likewise); d2 >> 1 = row
 *                                                                                       stride of dst in elements (0: d0)
 *      COPY_F32  src [d0] fp32, d0 % 4 == 0                 -> dst, same layout, the same bits (weights of two directions
 *                                                              side by side)
 *      ADD2      src, src2 [d0]                             -> dst = src + src2        (b_ih + b_hh; dst may be src)
 *      CAST_BF16 src [d0*d1] fp32, d0*d1 % 4 == 0           -> dst bf16, same layout, rounded to nearest even
 *                                                              (bf16 mode: weight operands)
 * CONV_T and TRANSPOSE write exactly the d0*d1 (five times that) elements named: with a row stride above d0 the columns
 * between the rows keep what they held.  A bf16 destination is rounded to nearest even.
 * Alignment (these kinds move whole vectors; DVAE_EINVAL otherwise, as for every other bad field, and nothing is launched):
 * COPY_F32 src and dst 16 bytes; CAST_BF16 src 16 bytes, dst 8 bytes; LSTM_PACK src, dst and dst2 16 bytes.  CONV_T,
 * TRANSPOSE and ADD2 go element by element and take any fp32 / bf16 aligned address.
 * `descs` is a HOST array of 1 <= n <= 72 entries (copied into the launch); the device buffers are the caller's.  A
 * descriptor is worked on by ceil(elements / 8192) workgroups, at most 512. */
#define DVAE_REPACK_CONV_T 0
#define DVAE_REPACK_LSTM_PACK 1
#define DVAE_REPACK_TRANSPOSE 2
#define DVAE_REPACK_ADD2 3
#define DVAE_REPACK_CAST_BF16 4
#define DVAE_REPACK_COPY_F32 5
typedef struct {
  int kind, d0, d1, d2;
  const void* src;
  const void* src2;
  void* dst;
  void* dst2;
} dvae_repack_desc_t;
int dvae_repack_all(const dvae_repack_desc_t* descs, int n, void* stream);

/* ---- W_hh-resident persistent recurrence (nn.LSTM at disentangled_vae.py:172,193; H = 512 / 1024) ----
 * Exists for: DVAE_MODE_BF16, forward and backward, (H/32) * ceil(N/32) <= CU count; DVAE_MODE_F32X3, FORWARD only (three
 * bf16 planes of W_hh resident, h handed over as three planes), N <= 128 (the backward recurrence streams the 4H-wide
 * gate gradients, which no residency shrinks: it stays on the per-frame kernels).
 * dvae_lstm_pers_supported: 1 when a call with (N, H, packed_mode = mode, pass) would take the persistent launch on the
 *   current device (given a workspace), else 0.
 * dvae_lstm_pers_ws_bytes: size of the synchronisation workspace (flags + sticky error record + the flags' epoch + exchange
 *   ring: two slots in use, four sized) for (N, H); 0 when the shape has no persistent kernel.
 * dvae_lstm_pers_check: SYNCHRONISES `stream`, then returns DVAE_ELAUNCH if a bounded wait of any persistent launch on
 *   this workspace gave up since the last check (info4 = {code 1 fwd / 2 bwd, workgroup, step, wave}; the outputs of
 *   that launch are garbage), DVAE_OK otherwise.  Not capturable; call it wherever the host synchronises anyway.
 * dvae_lstm_pers_selftest: a forward launch in which workgroup `drop_bid` never publishes — every waiter must give up
 *   within dir->pers_timeout_us and dvae_lstm_pers_check must then report it (tests/test_hip_lstm_pers.py). */
int dvae_lstm_pers_supported(int N, int H, int mode, int bwd);
int64_t dvae_lstm_pers_ws_bytes(int N, int H);
int dvae_lstm_pers_check(void* ws, int* info4, void* stream);
/* device address of the sticky error word of workspace `ws` (non-zero from the first bounded wait that gave up until
 * dvae_lstm_pers_check reported it): the `skip_if_nonzero` argument of dvae_adam_flat_dev */
const unsigned* dvae_lstm_pers_err_word(void* ws);
int dvae_lstm_pers_selftest(const dvae_lstm_dir_t* dir, int T, int N, int H, int64_t ldh, int drop_bid, void* stream);

int dvae_lstm_seq_fwd(const dvae_lstm_dir_t* dirs, int ndir, int T, int N, int H, int64_t ldh, void* stream);
int dvae_lstm_seq_bwd(const dvae_lstm_dir_t* dirs, int ndir, int T, int N, int H, int64_t ldh, void* stream);
/* launches of global steps [step_begin, step_end) only (H a multiple of 512, packed weights); the `dirs` entries may be
 * two directions of one layer or, with step_shift, two stacked layers of equal H, N, T and ldh */
int dvae_lstm_seq_fwd_range(const dvae_lstm_dir_t* dirs, int ndir, int T, int N, int H, int64_t ldh,
                            int step_begin, int step_end, void* stream);
int dvae_lstm_seq_bwd_range(const dvae_lstm_dir_t* dirs, int ndir, int T, int N, int H, int64_t ldh,
                            int step_begin, int step_end, void* stream);

/* ---- reparameterise + latent assembly (disentangled_vae.py:222-228, 252-272) ----
 * style[N,2S], content[N,2Cn] with N = 2*Bh (x1 rows then x2 rows); eps_c[N,Cn] (null => z = mu), eps_s[Bh,S].
 * Outputs: z[N,S+Cn], q_mu[N,S+Cn], q_lv[N,S+Cn] (rows [0,Bh) = q_z1, [Bh,N) = q_z2), s_mu[Bh,S], s_lv[Bh,S].
 * The x2 style head is detached (:257-258): its gradient rows are written as zero.
 */
int dvae_latent_fwd(const float* style, const float* content, const float* eps_c, const float* eps_s,
                    float* z, float* q_mu, float* q_lv, float* s_mu, float* s_lv,
                    int Bh, int S, int Cn, void* stream);
int dvae_latent_bwd(const float* style, const float* content, const float* eps_c, const float* eps_s,
                    const float* dz, const float* dq_mu, const float* dq_lv, const float* ds_mu,
                    const float* ds_lv, float* dstyle, float* dcontent, int Bh, int S, int Cn, void* stream);

/* ---- KL reduction (disentangled_vae.py:320-323): out[0] = scale * sum(1 + lv - mu^2 - exp(lv)) ---- */
int dvae_kl_fwd(const float* mu, const float* lv, float* out, int64_t n, float scale, void* stream);
/* dmu = g*scale*(-2mu), dlv = g*scale*(1-exp(lv)); g = *gout (device scalar) */
int dvae_kl_bwd(const float* mu, const float* lv, const float* gout, float* dmu, float* dlv,
                int64_t n, float scale, void* stream);

/* ---- L1 reconstruction loss, reduction='sum' (disentangled_vae.py:314-318): out[0] = scale*sum|x-y| ----
 * ws: >= dvae_l1_ws_bytes(n). */
int64_t dvae_l1_ws_bytes(int64_t n);
int dvae_l1_sum_fwd(const float* x, const float* y, float* out, void* ws, int64_t n, float scale, void* stream);
/* dy = -sign(x-y) * g * scale */
int dvae_l1_sum_bwd(const float* x, const float* y, const float* gout, float* dy, int64_t n, float scale,
                    void* stream);

/* ---- the whole loss_functionGVAE2 (disentangled_vae.py:310-327) in two launches forward, one backward ----
 * out8 = (LOSS, L1(x1,recon1), L1(x2,recon2), L1(x1,recon1_hat), L1(x2,recon2_hat), KL_z1, KL_z2, KL_style) with
 *   L1(x, r) = l1_scale * sum|x - r|                      (l1_scale = 1 / batch_size: F.l1_loss(sum).div(batch_size))
 *   KL_zk    = kl_scale * sum(1 + lv - mu^2 - exp(lv))   (kl_scale = -0.5 / rows of q_zk_mu: torch.mean over the batch)
 *   KL_style = style_scale * sum(...)                     (report only)
 *   LOSS     = mse_cof * (((L1_1 + L1_2) + L1_3) + L1_4) + kl_cof * (KL_z1 + KL_z2)
 * bwd: g8 = gradient w.r.t. out8 (a device vector: no host round trip); any output pointer may be null (not needed). */
typedef struct {
  const float *x1, *x2, *recon1, *recon2, *recon1_hat, *recon2_hat;   /* [n] each, 16-byte aligned */
  const float *q1_mu, *q1_lv, *q2_mu, *q2_lv;                          /* [nq] each */
  const float *s_mu, *s_lv;                                            /* [ns] each */
  int64_t n;
  int nq, ns;
  float l1_scale, kl_scale, style_scale, mse_cof, kl_cof;
} dvae_loss_desc_t;
int64_t dvae_loss_ws_bytes(int64_t n);
int dvae_loss_fwd(const dvae_loss_desc_t* desc, float* out8, void* ws, void* stream);
int dvae_loss_bwd(const dvae_loss_desc_t* desc, const float* g8, float* d_recon1, float* d_recon2, float* d_recon1_hat,
                  float* d_recon2_hat, float* d_q1_mu, float* d_q1_lv, float* d_q2_mu, float* d_q2_lv, float* d_s_mu,
                  float* d_s_lv, void* stream);

/* ---- the same loss with its two weights ON THE DEVICE and per-dimension free bits (Kingma et al. 2016) ----
 * For a KL warm-up inside a captured step: a weight that is a kernel argument is baked into the graph, one that is read
 * from `coef` follows whatever the host last copied there.  desc->mse_cof and desc->kl_cof are IGNORED.
 * q*_mu / q*_lv are row-major [rows, D] blocks, rows = nq / D.  With lambda = free_bits:
 *   kl_dim_k[j] = kl_scale * sum_i (1 + lv_ij - mu_ij^2 - exp(lv_ij))     (kl_scale = -0.5 / rows: the batch mean, in nats)
 *     each term in fp32 as dvae_loss_fwd computes it, the rows added in float64 in row order by the one thread that owns
 *     the column, one rounding at the store; no atomics: two calls give the same bits.
 *   gate_k[j]   = kl_dim_k[j] > lambda[j] ? 1 : 0   (STRICT: a dimension exactly at lambda is free; all 1 without free_bits)
 *   aux[k]      = sum_j max(lambda[j], kl_dim_k[j]), in float64 in dimension order, rounded once; without free_bits
 *                 aux[0], aux[1] are out8[5], out8[6] themselves
 *   out8[1..7]  the raw, unclamped terms: bit-identical to dvae_loss_fwd's on the same inputs, free bits or not
 *   out8[0]     = coef[0] * (((L1_1 + L1_2) + L1_3) + L1_4) + coef[1] * (aux[0] + aux[1]), in fp32 in that order (the
 *                 second product fused into the final sum, which is how dvae_loss_fwd's expression is compiled)
 * Without free_bits out8[0] and all ten gradients are bit-identical to dvae_loss_fwd / dvae_loss_bwd called with
 * mse_cof = coef[0], kl_cof = coef[1] (the same kernel bodies, instantiated on where the weights come from).
 * bwd, element (i, j) of half k: w = (g8[0] * coef[1] * gate_k[j] + g8[5 + k]) * kl_scale, d_mu = w * (-2 mu),
 *   d_lv = w * (1 - exp(lv)): on a free dimension nothing arrives from g8[0], what arrives from g8[5 + k] stays; on a
 *   penalised one w is dvae_loss_bwd's, bit for bit.  The reconstruction and style gradients are dvae_loss_bwd's with
 *   coef[0] for mse_cof; the null-output rules are dvae_loss_bwd's.  Forward is two launches, backward one, as before: the
 *   per-dimension work is done by the single final workgroup.
 * DVAE_EINVAL, nothing written: a null sched / coef / aux, D < 1, D > DVAE_LOSS_MAX_D, nq % D != 0, coef / free_bits / aux not
 *   4-byte aligned, and whatever dvae_loss_fwd / dvae_loss_bwd refuse. */
#define DVAE_LOSS_MAX_D 1024
typedef struct {
  const float* coef;       /* device float[8]: [0] mse_cof, [1] KL weight in effect; [2..7] reserved, read as written */
  const float* free_bits;  /* device float[D] nats per dimension (>= 0), or null: no free bits */
  int D;                   /* latent dimensions per row: nq % D == 0, 1 <= D <= DVAE_LOSS_MAX_D */
} dvae_loss_sched_t;
/* aux: device float[4 + 4*D], written by fwd, read by bwd:
 *   [0],[1]        KL_z1, KL_z2 as they enter LOSS (with free bits: sum_j max(lambda_j, kl_dim_k[j]))
 *   [2],[3]        dimensions of z1 / z2 that are free this step (kl_dim <= lambda), as floats
 *   [4 .. 4+2D)    kl_dim: per-dimension batch-mean KL in nats, z1 then z2
 *   [4+2D .. 4+4D) gate: 1.0 where the dimension is penalised (kl_dim > lambda), 0.0 where it is free */
int dvae_loss_fwd_sched(const dvae_loss_desc_t* desc, const dvae_loss_sched_t* sched, float* out8, float* aux, void* ws,
                        void* stream);
int dvae_loss_bwd_sched(const dvae_loss_desc_t* desc, const dvae_loss_sched_t* sched, const float* aux, const float* g8,
                        float* d_recon1, float* d_recon2, float* d_recon1_hat, float* d_recon2_hat, float* d_q1_mu,
                        float* d_q1_lv, float* d_q2_mu, float* d_q2_lv, float* d_s_mu, float* d_s_lv, void* stream);

/* ---- Adam over one flat parameter buffer (torch.optim.Adam at disentangled_vae.py:304) ----
 * g is multiplied by grad_scale first (1/world_size after a sum all-reduce). `step` is 1-based. */
int dvae_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float grad_scale, int step, void* stream);

/* Same update with every scalar that changes between steps kept ON THE DEVICE, so that a captured hipGraph replays a
 * correct Adam step and a learning-rate schedule needs no re-capture.  state: float[8], zero-initialised by the caller:
 *   [0] t (advanced by this call)   [1] 1 - beta1^t   [2] sqrt(1 - beta2^t)   [4] lr   [5] grad_scale
 * ([4], [5] written by the caller — optim.FlatAdam.sync_scalars — outside any capture).
 * skip_if_nonzero (optional): a device word; while it is non-zero the call changes NOTHING (no tick, no update, no clear).
 *   optim.FlatAdam passes the sticky error word of the persistent LSTM launches (dvae_lstm_pers_err_word): a launch that gave
 *   up a bounded wait left garbage gradients, and the weights / moments must not consume them before the host has looked.
 * clear: up to 8 ranges [lo, hi) of g (multiples of 4 elements) that are zeroed AFTER they were read — the
 *   optimizer.zero_grad() of the NEXT step (variational_base_vae.py:86) rides on this launch's pass over g.
 * tick: 1 advances t and the bias corrections first (one call per step); 0 applies the update of the CURRENT t to another
 *   slice of the buffers (a sharded optimizer — ddp.GradReducer(mode="rs_ag") — updates one slice per bucket; clear ranges
 *   are relative to the `g` passed).
 * n % 4 == 0. */
typedef struct {
  int64_t lo[8], hi[8];
  int n;
} dvae_ranges_t;
int dvae_adam_flat_dev(float* p, float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                       float* state, const unsigned* skip_if_nonzero, const dvae_ranges_t* clear, int tick, void* stream);

/* ---- global gradient-norm clipping and a non-finite step guard, on the device inside the (captured) step ----
 * Replaces torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) between loss.backward() and optimizer.step()
 * (variational_base_vae.py:68 and :69; the reference leaves room for it, its gradients being ordinary tensors there).
 * Three launches in place of dvae_adam_flat_dev's two-launch step:
 * dvae_grad_sumsq: one pass over g[0, n) (n % 4 == 0, 16-byte aligned), sum of g^2 accumulated in float64; every workgroup
 *   stores one float64 partial into ws (>= dvae_grad_sumsq_ws_bytes(n) bytes, 8-byte aligned).  No atomics: grid and
 *   summation order depend on n alone, the result is bit-identical from run to run.
 * dvae_grad_clip_finalize: adds the partials in a fixed order and, in float64, rounding once per store, fills clip (float[8],
 *   zero-initialised by the caller, [0] written by it — optim.FlatAdam.sync_scalars — outside any capture):
 *     [0] max_norm (+inf: measure and guard, never clip)
 *     [1] norm = state[5] * sqrt(sum): of the gradient Adam consumes (grad_scale included); +inf above FLT_MAX
 *     [2] coef = min(1, max_norm / (norm + 1e-6))          [3] eff = state[5] * coef: == state[5] bit for bit when coef == 1
 *     [4] 1 while this step is skipped: the sum is not finite (<=> some element is not: the square of a finite float32
 *         cannot overflow a double) and guard_nonfinite != 0; else 0
 *     [5] skipped steps so far     [6] clipped steps so far (coef < 1)     [7] 1 when the sum is not finite, guarded or not
 *   `state` is dvae_adam_flat_dev's; n is the n given to dvae_grad_sumsq.  While *skip_if_nonzero != 0 it changes nothing.
 * dvae_adam_flat_dev_clip: dvae_adam_flat_dev reading clip[3] in place of state[5]; while clip[4] != 0 t does not advance
 *   and p, m, v are not written, but the `clear` ranges of g are still zeroed (the next backward accumulates into them). */
int64_t dvae_grad_sumsq_ws_bytes(int64_t n);
int dvae_grad_sumsq(const float* g, int64_t n, void* ws, void* stream);
int dvae_grad_clip_finalize(const void* ws, int64_t n, const float* state, float* clip,
                            const unsigned* skip_if_nonzero, int guard_nonfinite, void* stream);
int dvae_adam_flat_dev_clip(float* p, float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                            float* state, const unsigned* skip_if_nonzero, const dvae_ranges_t* clear, int tick,
                            const float* clip, void* stream);

/* ---- exponential moving average of the weights, on the device inside the (captured) step ----
 * New functionality (the reference keeps the last iterate only).  Two launches after the Adam launch(es) of a full step:
 * dvae_ema_tick: one small workgroup decides whether this step's update is applied and with what weight.  ema_state is
 *   float[8], zero-initialised by the caller, [0] and [3] written by it — optim.FlatAdam.sync_scalars — outside any capture:
 *     [0] decay, in [0, 1)
 *     [1] k, the number of updates applied so far (a float: exact up to 2^24 updates)
 *     [2] w = 1 - d_k, the weight of the last update
 *     [3] warm-up: non-zero switches the ramp below on
 *     [4] 1 while this step's update is applied, 0 while it is skipped
 *     [5..7] reserved, never written
 *   The step is skipped while *skip_if_nonzero != 0 (optional; the word dvae_adam_flat_dev gets) or, with clip_or_null given
 *   (dvae_grad_clip_finalize's clip), while clip[4] != 0: [4] <- 0 and nothing else changes.  Otherwise k <- k + 1, [4] <- 1,
 *     d = warm-up ? min(decay, (1 + k) / (10 + k)) : decay      in float64 from the float32 decay, with the NEW k
 *     w = (float)(1.0 - d)                                      rounded once
 *   (the first warm-up update has d = 2/11: the average follows the weights instead of holding on to the initial values).
 * dvae_ema_update: while ema_state[4] != 0, ema[i] <- fmaf(w, p[i] - ema[i], ema[i]) with w = ema_state[2], for i in [0, n);
 *   while ema_state[4] == 0 nothing is written.  p is only read.  n % 4 == 0, both pointers 16-byte aligned, the buffers do
 *   not overlap; anything else is DVAE_EINVAL.  8 bytes read and 4 written per element, no atomics, no state shared between
 *   workgroups: bit-identical from run to run.  An element with p[i] == ema[i] bit for bit keeps its bits (p - ema is +0
 *   and w * 0 + ema is ema; the one exception is ema == p == -0.0, which becomes +0.0, and inf / NaN, which become NaN).
 * dvae_swap_f32: a[i] <-> b[i] for i in [0, n), bits moved and never computed with; same rules for n, alignment and overlap.
 *   optim.FlatAdam.swap_ema exchanges the weights and their average with it, in place: no temporary, no view changes. */
int dvae_ema_tick(float* ema_state, const unsigned* skip_if_nonzero, const float* clip_or_null, void* stream);
int dvae_ema_update(float* ema, const float* p, int64_t n, const float* ema_state, void* stream);
int dvae_swap_f32(float* a, float* b, int64_t n, void* stream);

/* x[0, n) = 0(16-byte aligned): optimizer.zero_grad() (variational_base_vae.py:86) and the outputs that split-k
 * contractions accumulate into atomically, zeroed by a launch of their own right in front of the accumulation. */
int dvae_zero_f32(float* x, int64_t n, void* stream);

/* out = a + b (+ c when non-null): the sum of the gradients of a tensor with several consumers — x feeding both
 * latent heads (disentangled_vae.py:212-215), the decoder output feeding the postnet, its residual and the loss
 * (variational_base_vae.py:292-293).  n % 4 == 0, 16-byte aligned. */
int dvae_sum_f32(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream);

/* ---- layout plumbing ----
 * dvae_mel_to_frames: x1,x2 [Bh,C,T] (torch layout, variational_base_vae.py:81-82) -> X[T, 2*Bh, C]; x2 may be
 *   null (then N = Bh).  dvae_frames_to_mel is the inverse ([T,N,C] -> out[N,C,T]).
 * dvae_permute_102: in[A,B,C] -> out[B,A,C]
 * dvae_colsum_add: out1[c] += sum_r X[r,c] (and out2 if non-null); X row stride ld; X fp32 or (x_bf16) bf16.
 * dvae_transpose: in[R,C] -> out[C,R]
 */
int dvae_mel_to_frames(const float* x1, const float* x2, void* X, int Bh, int C, int T, int out_bf16, void* stream);
int dvae_frames_to_mel(const float* X, float* out, int N, int C, int T, void* stream);
int dvae_permute_102(const float* in, float* out, int A, int B, int C, void* stream);
int dvae_colsum_add(const void* X, float* out1, float* out2, int R, int C, int64_t ld, int x_bf16, void* stream);
/* the same WITHOUT atomics (round 6): row blocks store partial sums into `ws`, the last workgroup of a column block to arrive
 * adds them up in row-block order and is the one writer of out[c] — run-to-run bit-identical.  ws: >= dvae_colsum_ws_bytes(R, C)
 * bytes, 16-byte aligned, its first 4096 bytes ZERO before the first call (every call leaves them zero); one ws per stream
 * that may have such a launch in flight */
int64_t dvae_colsum_ws_bytes(int R, int C);
int dvae_colsum_add_ws(const void* X, float* out1, float* out2, int R, int C, int64_t ld, int x_bf16, void* ws, void* stream);
int dvae_transpose(const float* in, float* out, int R, int C, void* stream);
/* dU = dZ * act'(Z), Z = activation OUTPUT (ReLU after enc_linear, disentangled_vae.py:211); dU may alias dZ */
/* Y = act(Y) in place (used after a split-K Linear) */
int dvae_act_fwd(float* Y, int64_t n, int act, void* stream);
int dvae_act_bwd(const float* dZ, const float* Z, float* dU, int64_t n, int act, void* stream);

/* ---- input pipeline on the device (SpeechDatasetGVAE.__getitem__, preprocessing/dataset.py:93-114, for a whole batch)
 * mels[n_utt, C, Lmax] padded store, lens[n_utt]; out[i] = crop of utterance utt[i] at frame off[i], T frames,
 * right-zero-padded when the utterance is shorter (:100-101). */
int dvae_gather_crop(const float* mels, const int* lens, const int* utt, const int* off, float* out, int n,
                     int C, int T, int Lmax, void* stream);

/* ---- inference: mel -> mel conversion plumbing (voice_conversion_mel, variational_base_vae.py:269-298; chunking_mel :335-348)
 * dvae_mel_to_chunks: mel[C,L] -> out[n,C,T], n = L/T + 1, tail zero-padded (an all-zero chunk when L % T == 0).
 * dvae_chunks_to_mel: in[n,C,T] -> out[C, n*T] (torch.cat of the chunks along time), optional clamp to [lo,hi] (:296).
 * dvae_conversion_latents: z_src[k] = [mean_k style_mu(src) | content_mu(src)[k]], z_conv[k] = [mean style_mu(trg) | same] (:281-285).
 * dvae_mul_div: out = a * (b / c)  (spectral detail, :301). */
int dvae_mel_to_chunks(const float* mel, float* out, int C, int L, int T, int n, void* stream);
int dvae_chunks_to_mel(const float* in, float* out, int n, int C, int T, float lo, float hi, int clamp, void* stream);
int dvae_conversion_latents(const float* src_style, const float* src_content, const float* trg_style,
                            float* z_src, float* z_conv, int n, int m, int S, int Cn, void* stream);
int dvae_mul_div(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream);

/* ---- inference: whole utterances through overlapped windows (in place of chunking_mel, variational_base_vae.py:335-348, and
 * of the per-chunk latents and torch.cat of voice_conversion_mel, :269-298, which join nothing at a chunk border).
 * A batch of utterances lies packed in mels [C, ld]: utterance u owns columns [col0, col0 + L).  Two int32 device tables:
 *   utt_table[nutt][4] = {col0, L, win0, nwin}   col0 increasing with u; windows win0 ... win0 + nwin - 1 are u's
 *   win_table[nwin][2] = {utt, frame0}           frame0 increasing inside an utterance; utt < 0: a padding window
 * (dvae_amd.convert.flat_plan writes them).
 * dvae_mel_to_windows: out[w][c][j] = mels[c][col0 + frame0 + j] while frame0 + j < L, else 0; a padding window is all zeros.
 *   A pure copy: columns that no utterance owns are never read.
 * dvae_window_latents: sums [G][K] float64 and counts [G] int64 as dvae_group_sum_f64 leaves them for the style heads (K = 2 S,
 *   the first S columns style_mu).  z[w][:S] = fp32((1 - mix) sums[g_src[w]] / counts[g_src[w]] + mix sums[g_trg[w]] /
 *   counts[g_trg[w]]) in float64, rounded once (the compiler may fuse the last multiply and add); z[w][S:] = content[w][:Cn],
 *   bits copied (content [nwin][2 Cn] = mu | logvar).  mix = 1: conversion, mix = 0: the source's own mean style, 0 <= mix <= 1.
 *   A window with g_src < 0 or g_trg < 0 is a row of zeros.  counts live on the device: the caller makes sure that no group
 *   in use is empty (dvae_amd.convert refuses it before the launch).
 * dvae_windows_overlap_add: out[c][col0 + t], t < L, from y [nwin][C][T]: where ONE window covers frame t its value's bits;
 *   elsewhere num = sum w[t - frame0] y[win][c][t - frame0], den = sum w[t - frame0] over the covering windows in window
 *   order, float64, out = fp32(num / den); then the optional clamp to [lo, hi] (:296).  One thread per output element, no
 *   atomics: two launches give the same bits.  Columns that no utterance owns are not written.  w [T] fp32, positive.
 * Null pointers, sizes < 1, a mix outside [0, 1] or lo > hi return DVAE_EINVAL and launch nothing. */
int dvae_mel_to_windows(const float* mels, int64_t ld, const int* utt_table, const int* win_table, float* out, int nwin,
                        int C, int T, void* stream);
int dvae_window_latents(const float* content, const double* sums, const int64_t* counts, const int* g_src, const int* g_trg,
                        double mix, float* z, int nwin, int S, int Cn, int K, void* stream);
int dvae_windows_overlap_add(const float* y, const int* utt_table, const int* win_table, const float* w, float* out,
                             int64_t ld, int nutt, int C, int T, float lo, float hi, int clamp, void* stream);

/* ---- over-smoothing of conversions: global variance, modulation spectrum and its postfilter (the
 * reference has no counterpart).  Mels lie packed as for the window kernels above: x [C, ld], utt_table[nutt][4] = {col0, L,
 * win0, nwin}.  Windows [nwin][C][D] are what dvae_mel_to_windows cuts with T = D; D even, DVAE_MODSPEC_DMIN <= D <=
 * DVAE_MODSPEC_DMAX.  twiddle [D][2] float64 = {cos, sin}(2 pi j / D), a host table (dvae_amd.modspec.twiddle).
 * dvae_mel_gv: out[u][c] = {m, v}, float64: m the mean and v the population variance (divisor L) of x[c][col0 .. col0 + L), two
 *   passes, the mean first and the centred squares second; a wave per (u, c), lane l adds frames l, l + 64, ... in index order,
 *   then a fixed tree over the wave: partition and order depend on L alone.  An entry with L < 1 or outside [0, ld) gives NaN
 *   and reads nothing.
 * dvae_modspec_windows: per window w and bin c, d_t = y_t - mean_t(y) (no taper), Y_k = sum_t d_t e^{-2 pi i k t / D} for k = 1 ..
 *   D/2, the sums over t in float64 in index order, s_k = ln max(|Y_k|^2, DVAE_MODSPEC_FLOOR), rounded once to fp32 at the store.
 *   rows[w C + c] = s_1 .. s_{D/2} | s_1^2 .. s_{D/2}^2 (fp32, D columns; the squares are those of the stored values, taken in
 *   float64 and rounded once).  k = 0 is zero by construction and is nowhere.  A padding window (all zeros) gives rows of ln
 *   FLOOR: the reduction passes over them because no group lists them.
 * dvae_modspec_group_sum: sums[g][c][j] (float64, [G][C][D], overwritten) = the sum of rows[order[i] C + c][j] over i in
 *   [group_first[g], group_first[g + 1]), in that order starting from +0: in every bit the sequential float64 sum.  order
 *   [norder] int32 lists window indices group by group, group_first [G + 1] int32; an index outside [0, nwin) is passed over.
 *   Workgroup (g, c), thread j; only a group's own rows are read.
 * dvae_modspec_filter: mu_n, sigma_n (natural) and mu_g, sigma_g (generated), float64 [C][D/2]; a sigma below
 *   DVAE_MODSPEC_SIGMA_MIN counts as that.  Per window, bin and k >= 1:  s' = (1 - alpha) s + alpha (sigma_n / sigma_g (s - mu_g) +
 *   mu_n);  log-gain = (s' - s) / 2 clamped to +- max_gain_db ln 10 / 20;  Y'_k = Y_k exp(log-gain), the phase kept;  out_t = mean +
 *   (1 / D) sum_k c_k Re(Y'_k e^{2 pi i k t / D}), k in index order, c_k = 2, c_{D/2} = 1.  All float64, rounded once to fp32.
 *   alpha = 0 copies the input's bits.  out != windows.
 * One workgroup per window and tile of 16 bins; frames and twiddles staged once in LDS; no atomics: two launches give the same
 * bits.  Null pointers, sizes < 1, C > 65535, an odd or out-of-range D, alpha outside [0, 1], max_gain_db <= 0 or a float64
 * buffer that is not 8-byte aligned return DVAE_EINVAL and launch nothing. */
#define DVAE_MODSPEC_DMIN 8
#define DVAE_MODSPEC_DMAX 128
#define DVAE_MODSPEC_FLOOR 1e-30
#define DVAE_MODSPEC_SIGMA_MIN 1e-6
int dvae_mel_gv(const float* x, int64_t ld, const int* utt_table, int nutt, int C, double* out, void* stream);
int dvae_modspec_windows(const float* windows, int nwin, int C, int D, const double* twiddle, float* rows, void* stream);
int dvae_modspec_group_sum(const float* rows, const int* order, int norder, const int* group_first, int G, int nwin, int C,
                           int D, double* sums, void* stream);
int dvae_modspec_filter(const float* windows, int nwin, int C, int D, const double* twiddle, const double* mu_n,
                        const double* sigma_n, const double* mu_g, const double* sigma_g, double alpha, double max_gain_db,
                        float* out, void* stream);

/* ---- modulation-spectrum and global-variance loss of the train step (ops.SmoothingPenaltyFn) ----
 * The reference's loss_functionGVAE2 (disentangled_vae.py:310-327) is L1 plus KL; this ADDS the squared distance between the log
 * modulation spectra, and between the log global variances, of the reconstruction and of its own target (modulation-spectrum-
 * constrained training, Takamichi et al., in the form an autoencoder allows), forward and backward.  Added at 319 without a new
 * revision: purely additive.
 * y [N, C, T] fp32 dense, N = 2 Bh; its target x: row n < Bh is x1[n], otherwise x2[n - Bh], both [Bh, C, T] fp32 dense.  The
 * W = T / D windows of a row are disjoint, no taper.  floor > 0; eps_ms = D floor^2, eps_gv = floor^2.  twiddle: as above.
 *   per (row, window, bin): d_t = y_t - mean_t(y), Y_k = sum_t d_t e^{-2 pi i k t / D} for k = 1 .. H = D/2 (float64, t in index
 *     order, the twiddle at k t mod D), P_k = |Y_k|^2, s_k = ln(P_k + eps_ms), Delta_k = s_k - s^x_k
 *     L_ms = the mean of Delta^2 over all M = N W C H elements
 *   per (row, bin): m = the mean over the row's T frames, v = (1 / T) sum_t (y_t - m)^2, g = ln(v + eps_gv)
 *     L_gv = the mean of (g - g^x)^2 over N C
 * dvae_msloss_fwd (two launches) writes stats [5] = {L_ms, L_gv, msd_db = (10 / ln 10) sqrt(L_ms), gv_ratio_db = (10 / ln 10)
 *   mean(g - g^x), penalty = weights[0] L_ms + weights[1] L_gv}, each float64 rounded once.  weights: DEVICE pointer to
 *   {w_ms, w_gv}.  penalty (may be null): one more float that receives stats[4].  ws (dvae_msloss_ws_bytes(N, C) bytes, 8-byte
 *   aligned) receives three float64 partial sums per workgroup (row n, tile of 16 bins: index n ceil(C / 16) + tile) and per
 *   (row, bin) m and 2 (g - g^x) / (v + eps_gv) for dvae_msloss_bwd.  Orders: a workgroup's 256 threads add their (bin, k)
 *   items window by window and then go through a binary tree; m and v: lane j of 16 the frames j, j + 16, ..., then the xor
 *   tree 8 .. 1; the second launch: thread r of 256 the workgroups r, r + 256, ... from +0, then a binary tree.
 * dvae_msloss_bwd (one launch, the same grid) reads y, x1, x2 and ws as dvae_msloss_fwd left it and stores
 *     dy_t = gscale (w_ms dL_ms/dy_t + w_gv dL_gv/dy_t), float64 rounded once to fp32, one writer per element, with
 *     dL_ms/dd_t = (4 / M) sum_k Delta_k / (P_k + eps_ms) (Re Y_k cos th_kt - Im Y_k sin th_kt), th_kt = 2 pi k t / D, k in index
 *     order; dL_ms/dy_t = that minus its mean over the window;  dL_gv/dy_t = (1 / (N C)) 2 (g - g^x) / (v + eps_gv) (2 / T) (y_t - m)
 *   gscale: DEVICE pointer to the incoming gradient of the penalty; null: 1.  A zero result is stored as +0.0.  When the device
 *   values of both weights are exactly 0, dy is +0.0 everywhere whatever y and x hold: the feature only monitors.
 * No atomics; every order is a function of (C, T, D) alone: a row's dy depends on the other rows through M and N only, and two
 * launches give the same bits.  Null pointers (penalty and gscale aside), Bh < 1, C < 1, C > 65535, an odd or out-of-range D,
 * T % D != 0, !(floor > 0) (or a floor whose square is not: eps_gv must be positive), a twiddle or ws that is not 8-byte
 * aligned return DVAE_EINVAL and launch nothing (dvae_msloss_ws_bytes: -1 for N < 1 or such a C). */
int64_t dvae_msloss_ws_bytes(int N, int C);
int dvae_msloss_fwd(const float* y, const float* x1, const float* x2, int Bh, int C, int T, int D, double floor,
                    const double* twiddle, const float* weights, float* stats, float* penalty, void* ws, void* stream);
int dvae_msloss_bwd(const float* y, const float* x1, const float* x2, int Bh, int C, int T, int D, double floor,
                    const double* twiddle, const float* weights, const float* gscale, const void* ws, float* dy,
                    void* stream);

/* ---- mel front-end: preprocessing/utils.py:68-73 `melspectrogram` = lws STFT (1024/256, "speech" window)
 * -> |.| -> 80-mel projection (librosa.filters.mel) -> dB (:127-129) - ref_level_db -> normalise to [0,1] (:136-137).
 * The two contractions (frames x DFT basis, magnitudes x mel basis) are dvae_gemm_f32 launches; these are the passes around them.
 * dvae_stft_frames: frames[M, fsize] = window * signal zero-padded by `left` samples in front (lws pads fsize-hop, :82-103).
 * dvae_stft_magnitude: reim[rows, 2*nbp] (real block | imaginary block) -> mag[rows, nbp].
 * dvae_mel_db_normalize: mel[M, n_mels] (frame-major) -> out[n_mels, ld_out] at column col0 (the [80, L] layout of the .npy corpus);
 *   DVAE_EINVAL unless col0 >= 0 and col0 + M <= ld_out (the M columns must fit inside a row of out). */
int dvae_stft_frames(const float* wav, int64_t n, const float* window, float* frames, int M, int fsize, int hop,
                     int left, void* stream);
int dvae_stft_magnitude(const float* reim, float* mag, int64_t rows, int nbins_padded, void* stream);
int dvae_mel_db_normalize(const float* mel, float* out, int M, int n_mels, int64_t ld_out, int64_t col0,
                          float min_level, float ref_level_db, float min_level_db, void* stream);

/* ---- Griffin-Lim inverse of the mel front-end (frontend.py MelInverter): normalised mel -> amplitude -> non-negative
 * linear magnitude -> fast Griffin-Lim -> waveform.  Every frame of every utterance of a batch is one row; the two DFT
 * contractions per iteration are dvae_gemm_f32 launches (fp32, unsplit); these are the passes around them.
 * dvae_mel_denormalize: mel[n_mels, ld_in] (columns 0..L) -> amp[L, n_mels] = 10^((clip(mel,0,1) * -min_db + min_db + ref_db) / 20).
 * dvae_mel_nnls_pg: x[rows, nbp] (in: warm start, out: solution) <- `iters` projected-gradient steps
 *   x = max(0, x - step * M^T (M x - amp)), M given sparsely: filt_range[n_mels][2] = bin range [lo, hi) of each filter,
 *   bin_filt[nbp][2] / bin_w[nbp][2] = the (at most two) filters of each bin (-1: none).  nbp <= 1024, n_mels <= 128.
 * dvae_gl_init: reim[rows, 2*nbp] (real block | imaginary block) = mag * exp(i phase); phase NULL: zero phase.
 * dvae_gl_phase: a = rebuilt - momentum/(1+momentum) * prev (prev NULL: 0), reim = mag * a / |a| (mag where |a| = 0).
 * dvae_gl_segment_table (host): table[nseg][4] = {row0, frames M, sample0, n = (M - fsize/hop + 1) * hop} of utterances
 *   packed row-wise; DVAE_EINVAL when some M < fsize/hop, fsize % hop != 0, or hop / fsize not multiples of 4.
 * dvae_ola_gather: overlap-add of the synthesis frames y[rows, fsize] with `window` inside each segment (`segs`: the table
 *   above, in device memory); mode 0: out[rows, fsize] = the next windowed analysis frames of the length-n signals (zero
 *   outside [0, n)); mode 1: out[sample0 + t] = sample t, out_len = total samples.  norm: divide by the overlap-added
 *   squared window. */
int dvae_mel_denormalize(const float* mel, float* amp, int L, int n_mels, int64_t ld_in, float ref_level_db,
                         float min_level_db, void* stream);
int dvae_mel_nnls_pg(const float* amp, float* x, int64_t rows, int nbp, int n_mels, const int* filt_range,
                     const int* bin_filt, const float* bin_w, float step, int iters, void* stream);
int dvae_gl_init(const float* mag, const float* phase, float* reim, int64_t rows, int nbp, void* stream);
int dvae_gl_phase(const float* rebuilt, const float* prev, const float* mag, float* reim, int64_t rows, int nbp,
                  float momentum, void* stream);
int dvae_gl_segment_table(const int* frames, int nseg, int fsize, int hop, int64_t* table);
int dvae_ola_gather(const float* y, const int64_t* segs, int nseg, int64_t rows, const float* window, float* out,
                    int64_t out_len, int fsize, int hop, int mode, int norm, void* stream);

/* ---- corpus preprocessing (python -m dvae_amd.preprocess): preprocessing/encoder/audio.py:22-51 `preprocess_wav` on a
 * packed batch of utterances of any source rates and lengths, one launch per pass for the whole batch.  The bits of an
 * output depend only on its own utterance and rate (not on the batch, not on the run): fixed tap / summation orders, one
 * writer per element, no atomics.
 * dvae_resample_segment_table (host): segment s of n_in[s] samples at filter filt[s] (filters[nfilt][6] = {P, Q, taps,
 *   base, woff, 0}: ratio sr_new / sr_old = P / Q in lowest terms, `taps` weights per phase at woff + phase * taps,
 *   tap c of output t reads input floor(t Q / P) - base + c) -> table[nseg][6] = {in0, n_in, out0, n_out, n_valid, filt}
 *   with n_valid = floor(n_in P / Q) (resampy's int(n * ratio)), n_out = ceil(n_in P / Q) (librosa.resample fix=True),
 *   in0 / out0 packed offsets rounded up to multiples of 4; tiles[ntiles][2] = {segment, t0} every `tile` outputs
 *   (tiles NULL: count only).  Returns ntiles, DVAE_EINVAL on a bad filter id, n_valid < 1 (resampy raises) or
 *   more than max_tiles tiles.
 * dvae_resample_lds_floats (host): the LDS floats a DVAE_RESAMPLE_TILE-output tile of filter (P, Q, taps) stages;
 *   DVAE_EINVAL above 64 KB.  dvae_resample_batch takes the maximum over the batch's filters.
 * dvae_resample_batch: resampy.resample(x, sr_old, sr_new, filter="kaiser_best") (resampy/interp.py resample_f) per
 *   segment, with the float64 per-phase weights rounded to fp32 (frontend.resample_filter): y[out0 + t] = sum_c w * x
 *   in tap order, inputs outside [0, n_in) zero (the tap bounds of resampy), y = 0 for n_valid <= t < n_out.  tiles
 *   from dvae_resample_segment_table with tile = DVAE_RESAMPLE_TILE; x, y 16-byte aligned.
 * dvae_volume_normalize: audio.py:121-127 normalize_volume(y, target_dbfs, increase_only) on every segment of the
 *   resampled batch, in place: float64 sum of squares per DVAE_VOLUME_TILE-sample tile (part[ntiles]), per segment
 *   ms = sum over its tiles tile_first[s] .. tile_first[s+1] in order / n_out, gain = 10^((target - 10 log10 ms) / 20)
 *   (1 where increase_only and the change is < 0), y *= gain.  ms == 0: silent[s] = 1, gain 1 (the reference would
 *   write 0 * inf = NaN).  tiles from dvae_resample_segment_table with tile = DVAE_VOLUME_TILE; ms_out optional.
 * dvae_stft_frames_seg / dvae_mel_db_normalize_seg: dvae_stft_frames / dvae_mel_db_normalize on a packed batch (the same
 *   kernels: one utterance is one segment passed by value), with the dvae_gl_segment_table layout {row0, M, sample0, n}
 *   in device memory: frame rows of segment s are [row0, row0 + M) of signal wav[sample0, sample0 + n); its [n_mels, M]
 *   block of `out` starts at n_mels * row0. */
#define DVAE_RESAMPLE_TILE 256
#define DVAE_VOLUME_TILE 2048
int dvae_resample_segment_table(const int64_t* n_in, const int* filt, int nseg, const int64_t* filters, int nfilt,
                                int tile, int64_t* table, int64_t* tiles, int64_t max_tiles);
int dvae_resample_lds_floats(int64_t P, int64_t Q, int taps);
int dvae_resample_batch(const float* x, float* y, const int64_t* segs, const int64_t* filters, const float* weights,
                        const int64_t* tiles, int ntiles, int lds_floats, void* stream);
int dvae_volume_normalize(float* y, const int64_t* segs, int nseg, const int64_t* tiles, int ntiles,
                          const int64_t* tile_first, double* part, double target_dbfs, int increase_only, double* ms_out,
                          float* gain, int* silent, void* stream);
int dvae_stft_frames_seg(const float* wav, const int64_t* segs, int nseg, int64_t rows, const float* window,
                         float* frames, int fsize, int hop, int left, void* stream);
int dvae_mel_db_normalize_seg(const float* mel, float* out, const int64_t* segs, int nseg, int64_t rows, int n_mels,
                              float min_level, float ref_level_db, float min_level_db, void* stream);

/* ---- silence trimming (python -m dvae_amd.preprocess --trim): the stage of audio.py:78-118 `trim_long_silences` between
 * dvae_volume_normalize and the mel, on the same packed batch (segs[nseg][6], columns 2, 3 = out0, n_out; out0 a multiple
 * of 4).  The reference asks webrtcvad, window by window; that package's sub-band GMM is not restated here, so the
 * detector below is this project's own and its parity with webrtcvad is UNPINNED.  The smoothing
 * and the dilation around it are the reference's (moving average of 8, np.round, binary_dilation with ones(6 + 1)),
 * restated on integers.  Per utterance of n = n_out samples y:
 *   W = n / 480 windows of 30 ms (DVAE_VAD_WINDOW); the n % 480 samples behind them are dropped
 *   E_w = sum of the window's (y[i] - 0.97 y[i-1])^2 in float64 (DVAE_VAD_PREEMPH; y[-1] = 0 at the utterance's first
 *         sample only, the predecessor crosses window borders), 8 consecutive samples per lane in index order, then a
 *         fixed tree over the wave
 *   b_w = clamp(ilogb(E_w) + DVAE_VAD_BIN_OFFSET, 0, DVAE_VAD_BINS - 1), read from the exponent field (zero and
 *         subnormal E_w: 0)
 *   c(b) = windows with b_w <= b; b10 / b90 the smallest b with c(b) >= ceil(W / 10) / ceil(9 W / 10)
 *   t = max(DVAE_VAD_BIN_FLOOR, min(b10 + DVAE_VAD_BIN_ABOVE_P10, b90 - DVAE_VAD_BIN_BELOW_P90));  flag_w = b_w >= t
 *   mask_w = more than half of the DVAE_VAD_MA_WIDTH flags of [w - 3, w + 4] set (5 of 8; np.round(4 / 8) is 0)
 *   keep_w = any mask of [w - 3, w + 3] (DVAE_VAD_MAX_SILENCE + 1 wide); flags and masks outside [0, W) are 0
 *   dst_w = kept windows before w;  K = kept windows in all
 *   out[out0 + 480 dst_w + i] = y[out0 + 480 w + i] for every kept w: the kept windows back to back, 480 K samples, at
 *         the segment's own offset of a second buffer.  480 K is a multiple of 4, so there are no pad floats behind it;
 *         nothing else of `out` is written.
 * Three launches for the batch on `stream` (energies: a wave per window; mask: a workgroup per utterance, chunked over
 * any W; compaction: a wave per kept window), no floating-point atomics, one writer per element, nothing passed between
 * workgroups: an utterance's bits depend on that utterance alone.  Everything behind E_w is integer logic.
 * wins[nwin][2] = {segment, w} lists every window of the batch, segment by segment; win_first[nseg + 1] is the index of
 * each segment's first window in it (both int64, in device memory, built by the caller; the kernels ignore an entry that
 * does not fit segs).  Per window, at its index in wins: E (float64, optional), bins, flags (optional), keep, dst (int32);
 * per segment: t (optional), K (int32).  segs_host is the host's copy of segs, read before the launches.
 * DVAE_EINVAL, nothing launched: nseg < 0, nwin != sum of n_out / 480, a required pointer null, y == out, y or out not
 * 16-byte aligned, another pointer not aligned to its element, an out0 that is negative or no multiple of 4, n_out < 0.
 * nseg == 0 is a no-op. */
#define DVAE_VAD_WINDOW 480
#define DVAE_VAD_MA_WIDTH 8
#define DVAE_VAD_MAX_SILENCE 6
#define DVAE_VAD_PREEMPH 0.97
#define DVAE_VAD_BINS 96
#define DVAE_VAD_BIN_OFFSET 80
#define DVAE_VAD_BIN_FLOOR 66
#define DVAE_VAD_BIN_ABOVE_P10 3
#define DVAE_VAD_BIN_BELOW_P90 5
int dvae_vad_trim(const float* y, float* out, const int64_t* segs_host, const int64_t* segs, int nseg, const int64_t* wins,
                  int64_t nwin, const int64_t* win_first, double* E, int* bins, int* flags, int* keep, int* dst, int* t,
                  int* K, void* stream);

/* ---- mel-cepstral distortion (python -m dvae_amd.evaluate): preprocessing/MCD_calculate.py:54-103 `evaluate_mcd_wav`
 * (WORLD mel-cepstra of the voiced frames, fastdtw, mean frame distance along the path) restated on a packed batch
 * (DESIGN.md §4.6).  The three contractions of the feature pass are dvae_gemm_f32 launches (fp32, unsplit); these are the
 * passes around them and the alignment.  No atomics, one writer per output element, fixed orders: a pair's bits depend
 * neither on the batch nor on the run.
 * dvae_log_power: reim[rows, 2*nbp] (real block | imaginary block) -> power = Re^2 + Im^2, log_power = ln(max(power,
 *   floor)), both [rows, nbp], 0 in bins nb..nbp; nbp a multiple of 4, all three 16-byte aligned.
 * dvae_voicing_compact: one workgroup per utterance of `segs` (the dvae_gl_segment_table layout {row0, M, sample0, n} in
 *   device memory).  r[rows, ldr]: column 0 = the frame's autocorrelation r(0), columns 1..nlag = r at the voicing lags;
 *   gain[ldr]: r_w(0) / r_w(lag) of the analysis window at the same columns.  peak[row] = max over the lags of r * gain,
 *   / r(0) (0 where r(0) = 0); voiced[row] = r(0) > 0 and r(0) >= rel_power_min * (max r(0) over the utterance) and
 *   peak >= peak_min.  The first DVAE_MCD_DIM coefficients of the voiced rows of mc[rows, ldm] go to feats[row0 + k] in
 *   time order (k = rank among the utterance's voiced frames); count[s] = the number of voiced frames.  mc, feats
 *   16-byte aligned, ldm a multiple of 4.
 * dvae_dtw_batch: exact DTW of each pair p of pairs[npairs][4] = {x_row0, nx, y_row0, ny} over rows of DVAE_MCD_DIM floats
 *   of x and y: D(i,j) = d(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)), d = the float64 euclidean distance of the fp32
 *   rows, a tie to the first of the three in that order (fastdtw's); cost[p] = D(nx-1, ny-1), length[p] = cells on that
 *   path.  nx == 0 or ny == 0: cost NaN, length 0.  `pairs` in device memory and the same table in host memory
 *   (pairs_host), checked before the launch: DVAE_EINVAL when some pair has min(nx, ny) > DVAE_DTW_MAX_SHORT.  One
 *   workgroup per pair; x, y 16-byte aligned. */
#define DVAE_MCD_DIM 24
#define DVAE_DTW_MAX_SHORT 4096
int dvae_log_power(const float* reim, float* power, float* log_power, int64_t rows, int nb, int nbp, float floor,
                   void* stream);
int dvae_voicing_compact(const float* r, int ldr, int nlag, const float* gain, const float* mc, int ldm,
                         const int64_t* segs, int nseg, float peak_min, float rel_power_min, float* peak, int* voiced,
                         float* feats, int* count, void* stream);
int dvae_dtw_batch(const float* x, const float* y, const int64_t* pairs, const int64_t* pairs_host, int npairs,
                   double* cost, int64_t* length, void* stream);

/* ---- F0 contour and log-F0 error along the MCD alignment (python -m dvae_amd.evaluate --f0) ----
 * dvae_f0_viterbi replaces `pyworld.harvest` of preprocessing/WORLD_processing.py:29-38 `world_decompose` (F0 per 5 ms
 *   frame, 0 on unvoiced frames), whose log statistics are `logf0_statistics` (:178-185).  One workgroup per utterance of
 *   `segs`; r, gain, voiced as dvae_voicing_compact reads / writes them, nlag == DVAE_F0_STATES.  Every maximal run of
 *   voiced frames is tracked on its own by a Viterbi pass over the states j (lag lag_min + j) in float64 without fused
 *   multiply-add: s_k(j) = r[k][1+j] * gain[1+j] / r[k][0] - oct[j]; D = s at the run's first frame, then
 *   D_k(j) = s_k(j) + max_i (D_{k-1}(i) - jump_cost * |l2[j] - l2[i]|), the first maximal i on a tie; the first arg-max
 *   of the last D starts the traceback.  l2, oct: [DVAE_F0_STATES] float64 device tables.  back[rows, DVAE_F0_BACK_LD]
 *   bytes: scratch for the back-pointers (4-byte aligned).  lag[row] = lag_min + j (0 unvoiced); f0[row] =
 *   sample_rate / (lag + delta), delta the parabolic vertex of r * gain around the lag (0 at the first and last state or
 *   where the parabola is not concave, clamped to +-0.5), 0 unvoiced; lf0v[row0 + k] = ln f0 of the utterance's k-th voiced
 *   frame, the row dvae_voicing_compact gives that frame in feats; rows past count[s] are not written.
 * dvae_dtw_batch_f0 replaces nothing of its own: it is dvae_dtw_batch (the same kernel body, cost and length bit-identical,
 *   the same refusals) that also carries, the way the path length is carried, the sum over the path's cells of
 *   (lf0x[x_row0 + i] - lf0y[y_row0 + j])^2 -> sse[p] (float64 terms, fp32 running sum; NaN where cost is NaN). */
#define DVAE_F0_STATES 206
#define DVAE_F0_BACK_LD 208
int dvae_f0_viterbi(const float* r, int ldr, int nlag, const float* gain, const int* voiced, const int64_t* segs, int nseg,
                    const double* l2, const double* oct, double jump_cost, double sample_rate, int lag_min,
                    unsigned char* back, int* lag, float* f0, float* lf0v, void* stream);
int dvae_dtw_batch_f0(const float* x, const float* y, const float* lf0x, const float* lf0y, const int64_t* pairs,
                      const int64_t* pairs_host, int npairs, double* cost, int64_t* length, double* sse, void* stream);

/* ---- speaker-identity probe of the latents (python -m dvae_amd.probe) ----
 * dvae_softmax_ce replaces the loss of model/train_feature_selection.py:39-41 (`F.cross_entropy` on the classifier's
 *   output; the reference applies a softmax first, model/feature_selection.py:41, which this does not repeat) and the
 *   arg-max accuracy of :44-50.  logits [rows, ld] fp32, classes <= ld, ld % 4 == 0, classes <= DVAE_CE_MAX_CLASSES,
 *   logits / dlogits 16-byte aligned; labels [rows] int32.  One wavefront per row, the row read once:
 *     row_loss[r] = logsumexp(logits[r, :classes]) - logits[r, label]   (the row maximum subtracted first)
 *     row_pred[r] = arg-max over [0, classes), the lowest index on a tie
 *     dlogits[r, c] = grad_scale * (softmax - onehot) for c < classes, 0 for classes <= c < ld (the contractions behind
 *                     read whole ld-wide rows).  May be null (evaluation); may be `logits` itself (in place).
 *   A row whose label is negative (or >= classes) is IGNORED: row_loss 0, gradient row 0, not counted; row_pred is
 *   still its arg-max.  out (optional, 4 floats, written by a second, one-workgroup launch that adds the rows in a fixed
 *   order in float64): {sum of row_loss over the counted rows, counted rows, counted rows with row_pred == label,
 *   out[0] / out[1] (0 when nothing is counted)}.  No atomics: a row's outputs do not depend on the rest of the batch and
 *   two runs give the same bits.
 * dvae_scale_by: y[i] = x[i] * scale[0], i < n (n % 4 == 0; scale a DEVICE scalar: the incoming gradient of the mean
 *   loss in ops.SoftmaxCeFn.backward; y may be x). */
#define DVAE_CE_MAX_CLASSES 1024
int dvae_softmax_ce(const float* logits, const int* labels, float* dlogits, float* row_loss, int* row_pred, float* out,
                    int rows, int classes, int64_t ld, float grad_scale, void* stream);
int dvae_scale_by(const float* x, const float* scale, float* y, int64_t n, void* stream);

/* ---- GMM-UBM speaker verification of conversions (python -m dvae_amd.verify) ----
 * Replaces nothing of the reference (it has no speaker-verification score): Reynolds, Quatieri, Dunn (2000) on the
 * mel-cepstra of dvae_voicing_compact.  A diagonal-covariance mixture of K components over D dimensions is THREE fp32
 * tables, computed by the caller in float64 from (w, mu, var) and rounded once (the tables as rounded are the model):
 *   a[k] = ln w_k - 1/2 sum_d ln(2 pi var_kd),  mu[k][d],  prec[k][d] = 1 / var_kd.
 * Frame t is x[t * ldx + col0 + d], d < D: ldx >= col0 + D, nothing assumed of x beyond 4-byte alignment (feats
 * [rows, 24] is read in place with col0 = 1, D = 23).  Per frame, in fp32, the same device function in both entry points:
 *   l_kt  = a_k - 1/2 sum_d (x_td - mu_kd)^2 prec_kd      (d ascending, one fma per term)
 *   lse_t = m_t + ln sum_k exp(l_kt - m_t), m_t = max_k l_kt   (k ascending; finite however far the frame is)
 * dvae_gmm_estep: lse [N] and gamma [N, K] (gamma_tk = exp(l_kt - lse_t), fp32, formed as exp(l_kt - m_t) over the sum so
 *   that a row adds up to 1 within K 2^-23 however large |lse_t| is) are optional (null: not written);
 *   stats, K (1 + 2 D) + 1 doubles, is OVERWRITTEN: per component k the record {n_k = sum_t gamma_tk, f_kd = sum_t gamma_tk
 *   x_td (d < D), s_kd = sum_t gamma_tk x_td^2 (d < D)} at stats[k (1 + 2 D)], and sum_t lse_t in the last double.  Every
 *   term is formed in float64 from the fp32 gamma and x and every sum is float64 in a fixed order: a workgroup owns
 *   consecutive tiles of 256 / 128 / 64 frames (K <= 64 / <= 128 / above) and one thread per output walks their frames in
 *   order; the partition is a function of (N, K, D) alone; per-workgroup sums go to ws (dvae_gmm_ws_bytes(N, K, D) bytes,
 *   nothing behind them is touched) and a second launch adds them in index order.  No atomics: two calls, or a call
 *   without lse / gamma, give the same bits.  ws and stats 8-byte aligned.
 * dvae_gmm_score: segs [nseg][2] int64 {row0, count} marks contiguous rows of x; M <= 65535 models lie back to back
 *   (a [M][K], mu [M][K][D], prec [M][K][D]); out[s][m] = sum of lse_t under model m over segment s, float64, exactly
 *   0.0 for count = 0.  One workgroup per (segment, model): thread i adds frames i, i + 256, ... in that order, then the
 *   xor tree over the 64 lanes of a wave (offsets 32 .. 1) and the four waves in order, so a row of out has the same bits
 *   whatever else is in the batch and equals that sum of dvae_gmm_estep's own lse.  segs and out 8-byte aligned.
 * Null required pointers, N, K, D, M, nseg < 1, K > DVAE_GMM_MAX_K, D > DVAE_GMM_MAX_DIM, col0 < 0, ldx < col0 + D or a
 *   misaligned float64 / int64 buffer return DVAE_EINVAL and launch nothing (dvae_gmm_ws_bytes returns 0). */
#define DVAE_GMM_MAX_K 256
#define DVAE_GMM_MAX_DIM 32
size_t dvae_gmm_ws_bytes(int64_t N, int K, int D);
int dvae_gmm_estep(const float* x, int64_t ldx, int col0, int64_t N, int D, const float* a, const float* mu,
                   const float* prec, int K, float* lse, float* gamma, void* ws, double* stats, void* stream);
int dvae_gmm_score(const float* x, int64_t ldx, int col0, int D, const int64_t* segs, int nseg, const float* a,
                   const float* mu, const float* prec, int K, int M, double* out, void* stream);

/* ---- i-vector speaker embeddings (python -m dvae_amd.ivector) ----
 * Replaces nothing of the reference (its speaker encoder is out of scope): the total-variability model of Dehak et al.
 * (2011) on the UBM above.  Everything is float64 but the UBM's three fp32 tables and the frames.  T [K D][R] (row c D + d)
 * lives in the whitened space; P [K][R][R], P_c = T_c^T T_c, is computed by the caller in float64 (only j <= i is read).
 * dvae_gmm_utt_stats: one workgroup per segment {row0, count} of x (as dvae_gmm_score).  gamma is the fp32 posterior of
 *   dvae_gmm_estep, from the same device functions (the same bits).  n [nseg][K]: n_k = sum_t gamma_tk;
 *   f [nseg][K D]: g_kd = sum_t gamma_tk x_td, f_kd = (g_kd - n_k (double)mu_kd) sqrt((double)prec_kd) (product, difference,
 *   product: three roundings; the square root is correctly rounded).  Terms are formed in float64 and every sum is float64
 *   over t ascending, by one thread: a segment's rows have the same bits whatever else is in the batch.  count <= 0 writes
 *   +0.0 everywhere.  segs, n and f 8-byte aligned.
 * dvae_ivec_posterior: one workgroup per utterance u < U, everything on chip (LDS: 2 R (R + 1) + K + 320 doubles):
 *   L = I + sum_c n_uc P_c (c ascending, one fma per term from +0);  b = T^T f_u, b_r = ((p_0 + p_1) + p_2) + p_3 with p_q
 *   the sum over rows q, q + 4, ... (ascending, one fma per term from +0);  L = G G^T by columns, the inner products k
 *   ascending;  every right-hand side (b and, with S, the R columns of I) is solved by ONE thread, G y = r rows ascending,
 *   G^T x = y rows descending, so w has the same bits with and without S and ll;
 *   w [U][R] = L^-1 b;  S [U][R][R] = L^-1 + w w^T (optional; S_ij is column j's solve plus w_i w_j by one fma: symmetric
 *   within the inverse's error, NOT mirrored);  ll [U] = 1/2 sum_i b_i w_i - sum_i ln G_ii (optional; i ascending).
 *   All orders are a function of (K, D, R) alone.  An utterance with n = 0 and f = 0 gives exactly w = +0.0, S = I,
 *   ll = +0.0.  L >= I for finite n >= 0, so no pivot is non-positive; a non-finite input gives NaN in that utterance's
 *   outputs only.
 * dvae_ivec_accumulate: A [K][R][R] = sum_u n_uc S_u, C [K D][R] = sum_u f_u w_u^T, Ssum [R][R] = sum_u S_u, all OVERWRITTEN.
 *   The utterances are cut into groups of max(64, ceil(U / 8)) consecutive ones; one thread per output element walks a
 *   group in order (terms formed in float64: one product, one addition) and writes to the group's slot of ws
 *   (dvae_ivec_ws_bytes(U, K, D, R) bytes, nothing behind them is touched); a second launch adds the slots in index order.
 * No atomics: two calls give the same bits.  Null required pointers, U, K, D, R, nseg < 1, K > DVAE_GMM_MAX_K,
 *   D > DVAE_GMM_MAX_DIM, R > DVAE_IVEC_MAX_R, col0 < 0, ldx < col0 + D or a misaligned float64 / int64 buffer return
 *   DVAE_EINVAL and launch nothing (dvae_ivec_ws_bytes returns 0). */
#define DVAE_IVEC_MAX_R 64
int dvae_gmm_utt_stats(const float* x, int64_t ldx, int col0, int D, const int64_t* segs, int nseg, const float* a,
                       const float* mu, const float* prec, int K, double* n, double* f, void* stream);
int dvae_ivec_posterior(const double* n, const double* f, const double* T, const double* P, int U, int K, int D, int R,
                        double* w, double* S, double* ll, void* stream);
size_t dvae_ivec_ws_bytes(int U, int K, int D, int R);
int dvae_ivec_accumulate(const double* n, const double* f, const double* w, const double* S, int U, int K, int D, int R,
                         void* ws, double* A, double* C, double* Ssum, void* stream);

/* ---- latent report: pairwise posterior log-densities and their log-sum-exps (python -m dvae_amd.latents) ----
 * Replaces nothing of the reference (its only latent diagnostic is compute_KL_delta_VAE, model/disentangled_vae.py:333-345,
 * unused): the minibatch-weighted-sampling decomposition of Chen et al. (2018) taken over a whole corpus of N posteriors
 * N(mu_j, exp lv_j) with one sample z_i each.  Four fp32 tables [N, D] with leading dimension ld; as rounded they ARE the
 * model:
 *   z = mu + exp(lv / 2) eps,  a = -(ln 2 pi + lv) / 2,  h = exp(-lv) / 2
 * dvae_latent_tables: elementwise, mu, lv, eps -> z, a, h (expf of the device library; z by one fma; a by one addition to the
 *   fp32 constant ln(2 pi) / 2; the halvings are exact).  Columns D .. ld - 1 are neither read nor written.  N = 0: no-op.
 * dvae_latent_lse: t_ijd = a_jd - h_jd (z_id - mu_jd)^2 (dz = z - mu, q = dz dz, t = fma(-h, q, a)); style_ij = the sum of
 *   t_ijd over d < S, content_ij over S <= d < D (d ascending from +0, an empty block is 0), joint_ij = style_ij + content_ij.
 *   jobs [njobs][5] int64 {row0, nrows, col0, ncols, out0} (device, 8-byte aligned; jobs_host the same table on the host, read
 *   during the call): job k writes, for r < nrows, out[(out0 + r) ldo + c] = the log-sum-exp over j in [col0, col0 + ncols)
 *   of t_(row0 + r) j c for c < D, of style, content and joint at c = D, D + 1, D + 2; nothing else of out is written.
 *   A log-sum-exp is m + ln s, (m, s) the running maximum and the sum of exp(. - m): every column takes the maximum off
 *   before its exponential (e = exp(min(m, t) - max(m, t)); s = t > m ? s e + 1 : s + e, from (-inf, 0)), so a row however
 *   far from every column gives finite values.  A wave owns 64 rows, one per lane; the four waves of a workgroup take the
 *   quarters [w q, (w + 1) q), q = ceil(ncols / 4), of the job's columns in ascending order and are merged in wave order
 *   (m = max(m, m'); s = fma(s', exp(m' - m), s exp(m_old - m)), the earlier waves' pair primed); exponentials are
 *   v_exp_f32 of the argument times log2 e, the final logarithm is logf.  The partition is a function of (ncols, D) alone, a
 *   row's bits depend on nothing but its own row of z, the job's columns, D and S — not on the other rows or jobs of the
 *   launch — and there are no atomics: two launches give the same bits.  Rows and columns must lie inside the tables (the
 *   entry point does not know N).  A job with nrows = 0 writes nothing; a launch of such jobs only is a no-op.
 * Null pointers, D < 1, D > DVAE_LATENT_MAX_D, S < 0, S > D, ld < D, ldo < D + 3, njobs < 1, a misaligned jobs, or a job with
 *   a negative field or ncols < 1 return DVAE_EINVAL and launch nothing. */
#define DVAE_LATENT_MAX_D 64
int dvae_latent_tables(const float* mu, const float* lv, const float* eps, float* z, float* a, float* h, int64_t N, int D,
                       int64_t ld, void* stream);
int dvae_latent_lse(const float* z, const float* mu, const float* a, const float* h, int64_t ld, int D, int S,
                    const int64_t* jobs, const int64_t* jobs_host, int njobs, float* out, int64_t ldo, void* stream);

/* ---- latent map: exact matrix-free t-SNE and 1-NN search (python -m dvae_amd.latent_map) ----
 * Replaces, on the project's own latents, the 2-D projections the reference draws for its vendored speaker encoder
 * (preprocessing/encoder/visualizations.py:164-168, UMAP) and its per-speaker latent plots (model/plot.py:23-55); the
 * optimiser is scikit-learn's exact t-SNE (van der Maaten & Hinton 2008).  Added at 319 without a new revision: purely additive.
 * x [N, D] fp32, leading dimension ld, 1 <= D <= DVAE_LATENT_MAX_D; columns D .. ld - 1 are never read.  No N x N table is
 * stored: every pass recomputes d_ij = sum_d (x_id - x_jd)^2 in the difference form (dz = x_id - x_jd, acc = fma(dz, dz, acc),
 * d ascending from +0), so d_ij and d_ji are the same bits.  A launch computes the rows [row0, row0 + nrows) against all N
 * columns and writes those rows of its outputs only (nrows = 0: no-op).  A wave owns 64 rows, one per lane; the four waves
 * of a workgroup take the quarters [w q, (w + 1) q), q = ceil(N / 4), of the columns in ascending order and are combined in
 * wave order, ((w0 + w1) + w2) + w3.  Every order is a function of (N, D) alone and there are no atomics: a row's bits do not
 * depend on the other rows of the launch, and two launches give the same bits.  All calls are asynchronous on `stream`.
 * dvae_tsne_nn: d2min[i], arg[i] = the smallest d_ij and its j over the admissible j: j != i when group is null, otherwise
 *   group[j] != group[i] (group [N] int32).  Ties go to the lowest j; a row without an admissible j gets +inf and -1.
 * dvae_tsne_affinities: van der Maaten's search, per row, for the precision beta at which p_j ~ exp(-beta d'_j),
 *   d'_j = max(d_ij - d2min[i], 0), j != i, has entropy ln perplexity: S0 = sum exp(-beta d'), S1 = sum d' exp(-beta d')
 *   (fma), lnz = logf(S0), entropy = fma(beta, S1 / S0, lnz).  beta starts at 1, doubles (up to 2^100) or halves until
 *   bracketed, then bisects; a row stops when |entropy - ln perplexity| <= 1e-5 (scikit-learn's tolerance) and steps[i] is
 *   the number of evaluations it took.  After max_steps evaluations steps[i] = -1 and beta, lnz, entropy are the last
 *   evaluation's, all finite.  With d2min from dvae_tsne_nn (group null) the nearest neighbour contributes exp(0) = 1:
 *   lnz >= 0 and no exponent is positive.  N >= 2, 1 <= perplexity <= N - 1, max_steps >= 1.
 * dvae_tsne_forces: one gradient evaluation at y [N, 2].  Per pair, j != i:
 *   p = (exp(fma(-beta_i, d'_i, -lnz_i)) + exp(fma(-beta_j, d'_j, -lnz_j))) * fp32(1 / 2N),  d'_k = max(d_ij - d2min_k, 0),
 *   q = fma(dy1, dy1, dy0 dy0), dy = y_i - y_j,  w = rcp(1 + q).
 *   rows[i][0..7] = sum_j of p w dy0, p w dy1, w w dy0, w w dy1, w, and with want_kl = 1: p logf(p) over p > 0,
 *   -p log1pf(q) (= p ln w), p; zeros with want_kl = 0.  Exponentials are v_exp_f32 of the argument times log2 e.
 * dvae_tsne_update: Z = the sum of rows[.][4], and with kl non-null the three KL sums, in float64 in one fixed order (thread
 *   t of 256 adds the rows t, t + 256, ... ascending; the 256 partial sums are then added in thread order);
 *   *kl = sum p ln p - sum p ln w + ln Z sum p (double, 8-byte aligned, device).  Then scikit-learn's _gradient_descent rule,
 *   element by element: g = 4 fma(ex, A, -(R fp32(1 / Z))); gains = max(upd g < 0 ? gains + 0.2 : gains 0.8, 0.01);
 *   upd = fma(momentum, upd, -(lr (gains g))); y += upd.  y, upd, gains [N, 2].
 * Null required pointers, N < 1, N > INT_MAX, D outside 1 .. DVAE_LATENT_MAX_D, ld < D, a row range outside [0, N], want_kl
 *   outside {0, 1}, lr <= 0, momentum < 0, exaggeration <= 0, a misaligned kl, or (affinities) N < 2, a perplexity outside
 *   [1, N - 1] or max_steps < 1 return DVAE_EINVAL and launch nothing. */
int dvae_tsne_nn(const float* x, int64_t ld, int64_t N, int D, const int* group, int64_t row0, int64_t nrows, float* d2min,
                 int* arg, void* stream);
int dvae_tsne_affinities(const float* x, int64_t ld, int64_t N, int D, const float* d2min, float perplexity, int max_steps,
                         int64_t row0, int64_t nrows, float* beta, float* lnz, float* entropy, int* steps, void* stream);
int dvae_tsne_forces(const float* x, int64_t ld, int64_t N, int D, const float* beta, const float* d2min, const float* lnz,
                     const float* y, int want_kl, int64_t row0, int64_t nrows, float* rows, void* stream);
int dvae_tsne_update(const float* rows, int64_t N, float* y, float* upd, float* gains, float lr, float momentum,
                     float exaggeration, double* kl, void* stream);

/* ---- speaker adversary on the content latent (dvae_amd/adversary.py) ----
 * The reference has the classifier and its loss (model/feature_selection.py:5-43, a speaker classifier with a cross-entropy
 * loss) but never trains the encoder against it; this is the gradient-reversal remedy of Ganin & Lempitsky (2015), Chou et
 * al. (2018) for voice conversion.  Added at 319 without a new revision: purely additive.
 * The network is Linear(D, H) -> ReLU -> Linear(H, S) -> softmax cross-entropy over R rows, forward and backward in TWO
 * launches.  x [R, ldx] fp32 is read in place (columns D .. ldx - 1 never; 4-byte alignment is enough); labels [R] int32;
 * w1 [H, ldw1] (D <= ldw1 <= DVAE_ADV_MAX_D, ldw1 % 4 == 0, columns D .. ldw1 - 1 are padding: loaded with the row's 16-byte pieces, never used), b1 [H],
 * w2 [S, H], b2 [S]; w1 and w2 16-byte aligned.  coef: DEVICE pointer to the reversal weight lambda; inv_rows = 1 / R.
 * dvae_adv_rows, one workgroup per row r (all buffers dense: row_loss, row_pred [R]; h, g1 [R, H]; g2 [R, S]):
 *     h[r, j]     = relu(sum_d w1[j, d] x[r, d] + b1[j])                   d ascending from +0, one fma per term, then the bias
 *     logit_c     = sum_j w2[c, j] h[r, j] + b2[c]                         a wave per class: lane l adds the 16-byte pieces l,
 *                   l + 64, ... of the row in ascending order (fma), the 64 lanes by the xor tree 32 .. 1, then the bias
 *     row_loss[r] = logsumexp(logit) - logit[label]                        the row maximum taken off first (expf, logf)
 *     row_pred[r] = arg-max of the logits, the lowest index on a tie
 *     g2[r, c]    = inv_rows (softmax_c - onehot_c)                        softmax_c = expf(logit_c - max) * (1 / sum)
 *     g1[r, j]    = h[r, j] > 0 ? sum_c g2[r, c] w2[c, j] : +0             c ascending from +0, one fma per term
 *     dx[r, dx_col0 + d] = -(lambda * sum_j g1[r, j] w1[j, d])             eight runs of H / 8 consecutive j, each ascending (fma),
 *                   added in run order; dx [R, lddx], lddx >= dx_col0 + D: every OTHER column of the row is written +0.0 (the
 *                   gradient of a wider tensor whose columns dx_col0 .. dx_col0 + D - 1 are x; lddx = D, dx_col0 = 0: dense)
 *   A row whose label is negative or >= S is IGNORED (dvae_softmax_ce's rule): row_loss 0, its rows of g2, g1 and dx +0.0, not
 *   counted; h and row_pred are written all the same.  When the device value of lambda is exactly 0, dx is +0.0 everywhere
 *   whatever the row holds: a NaN in the adversary does not reach the model while it only monitors.
 * dvae_adv_params, one lane per element of dw2 [S, H], db2 [S], dw1 [H, ldw1], db1 [H]: the sum over the counted rows in
 *   ascending order from +0 (fma), STORED, not accumulated:
 *     dw2[c, j] = sum_r g2[r, c] h[r, j],  db2[c] = sum_r g2[r, c],  dw1[j, d] = sum_r g1[r, j] x[r, d],  db1[j] = sum_r g1[r, j]
 *   padding columns of dw1 get +0.0.  The four may all be null (evaluation): then only `out` is written.  One more workgroup
 *   writes out[4] = {sum of row_loss over the counted rows, counted rows, counted rows with row_pred == label,
 *   out[0] * inv_rows}, added in float64 in row order by one thread.
 * No atomics; every order is a function of (D, H, S) alone: a row's bits do not depend on the other rows, and two launches
 * give the same bits.  Null required pointers, R < 1, D outside 1 .. DVAE_ADV_MAX_D, H outside 64 .. DVAE_ADV_MAX_H or not a
 * multiple of 64, S outside 1 .. DVAE_CE_MAX_CLASSES, ldx < D, a bad ldw1, dx_col0 < 0, lddx < dx_col0 + D, a misaligned w1 /
 * w2, or some but not all of the four gradients null return DVAE_EINVAL and launch nothing. */
#define DVAE_ADV_MAX_D 64
#define DVAE_ADV_MAX_H 1024
int dvae_adv_rows(const float* x, int64_t ldx, const int* labels, const float* w1, int ldw1, const float* b1,
                  const float* w2, const float* b2, const float* coef, float inv_rows, int R, int D, int H, int S,
                  float* row_loss, int* row_pred, float* h, float* g2, float* g1, float* dx, int64_t lddx, int dx_col0,
                  void* stream);
int dvae_adv_params(const float* x, int64_t ldx, const int* labels, const float* h, const float* g2, const float* g1,
                    const float* row_loss, const int* row_pred, float inv_rows, int R, int D, int H, int S, float* dw1,
                    int ldw1, float* db1, float* dw2, float* db2, float* out, void* stream);

/* ---- total-correlation and shared-information penalty of the train step (ops.FactorPenaltyFn) ----
 * The reference's loss_functionGVAE2 (disentangled_vae.py:310-327) is L1 plus KL and has no term on the two figures the latent
 * report prints beside them; this ADDS the beta-TCVAE penalty of Chen et al. (2018) on the minibatch, forward and backward.
 * Added at 319 without a new revision: purely additive.
 * z, mu, lv [N, D] fp32, dense (the N = 2 Bh rows of a step, z an argument of its own); the S style columns first, the
 * D - S content columns behind.  With a_jd = -(ln(2 pi) / 2 + lv_jd / 2), h_jd = expf(-lv_jd) / 2 and
 *     t_ijd = a_jd - h_jd (z_id - mu_jd)^2          (dz = z - mu, q = dz dz, t = fma(-h, q, a): dvae_latent_lse's)
 *     style_ij, content_ij = the sums of t_ijd over d < S, d >= S   (the 64 lanes of a wave by the xor tree 32 .. 1)
 *     joint_ij = style_ij + content_ij
 * dvae_factor_fwd (two launches) writes L [N, D + 3]: per row i the log-sum-exp over j of t_i.d (d = 0 .. D - 1), style,
 *   content and joint, the maximum taken off before every exponential (expf, logf): a row far from every column keeps a
 *   finite L.  A per-dimension sum runs over the columns j = w, w + 4, ... in order for w = 0 .. 3 and adds the four in that
 *   order; a block's over j = l, l + 64, ... for l = 0 .. 63 and adds the 64 by the xor tree.  ws (dvae_factor_ws_bytes(N)
 *   bytes, 4-byte aligned) receives own_i = joint_ii.  stats [5] = {tc_style, tc_content, shared, mi, penalty}, means over the
 *   rows added in float64 in a fixed order (thread r of 256 the rows r, r + 256, ..., then a binary tree):
 *     tc_style = mean_i[(L_style - ln N) - sum_{d < S} (L_d - ln N)]      tc_content likewise over d >= S
 *     shared   = mean_i[L_joint - L_style - L_content + ln N]             mi = mean_i[own_i - (L_joint - ln N)]
 *     penalty  = weights[0] (tc_style + tc_content) + weights[1] shared
 *   weights: DEVICE pointer to {w_tc, w_sh}, the warm-up factor already applied.  penalty (may be null): one more float
 *   that receives stats[4], for a caller that keeps `stats` and hands the penalty on as a tensor of its own.
 * dvae_factor_bwd (one launch of 2 N workgroups: N own a row i and write dz [N, D], N own a column j and write dmu, dlv
 *   [N, D]) reads L as dvae_factor_fwd left it and recomputes t; nothing of size N x N is stored.  With
 *   p_A(j|i) = expf(A_ij - L_A(i)), c_joint = w_sh, c_style = c_content = w_tc - w_sh, c_d = -w_tc, each times gscale[0]
 *   (DEVICE pointer to the incoming gradient of the penalty; null: 1), and r = 2 h_jd (z_id - mu_jd):
 *     g_ijd = ((c_joint p_joint + c_block p_block(d)) + c_d p_d) / N
 *     dz[i, d] = sum_j -g r     dmu[j, d] = sum_i g r     dlv[j, d] = sum_i g (r (z_id - mu_jd) / 2 - 1 / 2)
 *   each sum in index order from +0, one fma per term.  When the device values of both weights are exactly 0, all three are
 *   +0.0 everywhere whatever the inputs hold: a NaN in the statistics does not reach the model while the feature only monitors.
 * No atomics; every order is a function of (N, D, S) alone: a row's L does not depend on which rows are in the launch beyond
 * the columns they are, and two launches give the same bits.  Null pointers (penalty and gscale aside), N outside 1 .. DVAE_FACTOR_MAX_N,
 * S < 1, D - S < 1 or D > DVAE_LATENT_MAX_D return DVAE_EINVAL and launch nothing (dvae_factor_ws_bytes: -1). */
#define DVAE_FACTOR_MAX_N 1024
int64_t dvae_factor_ws_bytes(int N);
int dvae_factor_fwd(const float* z, const float* mu, const float* lv, int N, int D, int S, const float* weights, float* L,
                    float* stats, float* penalty, void* ws, void* stream);
int dvae_factor_bwd(const float* z, const float* mu, const float* lv, const float* L, int N, int D, int S,
                    const float* weights, const float* gscale, float* dz, float* dmu, float* dlv, void* stream);

/* ---- held-out validation (model/variational_base_vae.py: validate) ----
 * The reference's test() (variational_base_vae.py:105-123) sums loss_functionGVAE2 (disentangled_vae.py:310-327) over the
 * test batches.  dvae_pair_metrics gives those eight terms PER PAIR: the reference's formulas with its batch_size set to 1,
 * so that the mean of the rows of a full batch is what dvae_loss_fwd reports for it, and a held-out set gives the same
 * numbers however it was batched (a ragged last batch included).  Layouts of DisentangledVAE.forward_full:
 *   x1, x2 [Bh, n_per]; rec, rec_hat [2 Bh, n_per] (x1 half first); q_mu, q_lv [2 Bh, D]; s_mu, s_lv [Bh, S]; out [Bh, 8]:
 *   out[b] = (LOSS, L1(x1[b], rec[b]), L1(x2[b], rec[Bh+b]), the same two on rec_hat, KL_1, KL_2, KL_style) with
 *   L1 = sum|x - r|, KL_1 / KL_2 = -0.5 sum_d(1 + lv - mu^2 - exp lv) over rows b / Bh + b of q_*, KL_style = -sum_s(...) over
 *   row b of s_*, LOSS = mse_cof (((L1_1 + L1_2) + L1_1hat) + L1_2hat) + kl_cof (KL_1 + KL_2).
 *   One workgroup of 256 threads per pair; float4 loads when x1, x2, rec, rec_hat are 16-byte aligned and n_per % 4 == 0,
 *   a scalar walk otherwise; any n_per, D, S >= 1.  The elementwise terms are fp32, as dvae_loss_fwd computes them; every
 *   accumulation is float64 in a fixed order (per thread, then a fixed tree), LOSS is combined in float64 from the unrounded
 *   sums, and each output rounds once, at the store.  No atomics: two launches give the same bits.
 * dvae_group_sum_f64: rows [P, K] fp32 (K <= 256), group [P] int32; sums [G + 1, K] float64, counts [G + 1], bad [G + 1] int64 are
 *   ACCUMULATED INTO (one set of buffers spans all batches of a pass; the caller zeroes them first); row G is the total.
 *   Row p counts when 0 <= group[p] < G and its K values are all finite: it is added to sums[group[p]] and sums[G], and
 *   counts[group[p]], counts[G] grow by one.  Otherwise it enters no sum: a row with a value that is not finite adds one to
 *   bad[group[p]] and to bad[G], a row whose group is out of range to bad[G] alone.  One workgroup per output row, thread k
 *   walks p = 0 ... P - 1 in order: each sums[g][k] equals, in every bit, the sequential float64 sum (old value first).
 * Null pointers or sizes < 1 return DVAE_EINVAL and launch nothing. */
int dvae_pair_metrics(const float* x1, const float* x2, const float* rec, const float* rec_hat, const float* q_mu,
                      const float* q_lv, const float* s_mu, const float* s_lv, float* out, int Bh, int64_t n_per, int D,
                      int S, float mse_cof, float kl_cof, void* stream);
int dvae_group_sum_f64(const float* rows, const int* group, int P, int K, int G, double* sums, int64_t* counts, int64_t* bad,
                       void* stream);

/* ---- opt-in per-family kernel timing with HIP events on the launch stream (bench.py roofline) ----
 * family: 0 = off, 1 = GEMM/conv contraction kernel, 2 = LSTM step kernels, 3 (DVAE_PROF_AUDIO) = the launches of
 * dvae_volume_normalize (tags 0, 1, 2 in launch order) and of dvae_vad_trim (tags 3, 4, 5), for scripts/vad_cost.py.
 * dvae_prof_collect: synchronises the recorded events, returns total ms, launch count and algorithmic FLOPs. */
#define DVAE_PROF_AUDIO 3
int dvae_prof_enable(int family);
int dvae_prof_collect(double* total_ms, int64_t* launches, double* flops);
/* the same, split by kernel instantiation (call BEFORE dvae_prof_collect, which resets).  Contraction family: tag =
 * a_kcontig | b_kcontig << 1 | NTW << 2 | BK << 4 | WG << 10 | mode << 13 | tap_mode << 15, i.e. the template arguments
 * of gemm_f32_kernel<A_KC, B_KC, NTW, BK, WG, MODE>; bytes = algorithmic operand bytes (each element once).  Returns the
 * number of distinct tags (<= max_tags written). */
int dvae_prof_collect_tags(unsigned* tags, double* ms, int64_t* launches, double* flops, double* bytes, int max_tags);
#ifdef __cplusplus
}
#endif
#endif
