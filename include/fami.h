/* fami.h -- C ABI of libfami_hip.so: the MI355X (gfx950) kernels behind the
 * FAMI-Pose temporal-alignment training hot path.
 *
 * The reference has NO native FFI on this path: its compute is
 * reached through torch.nn modules, torchvision's registered op
 * torchvision::deform_conv2d and kornia.geometry.warp_affine.  Each entry point
 * below therefore names the reference *call site / module* it replaces
 * (file:line relative to the reference tree).  A reference maintainer binds
 * them with ctypes; fami-pose_amd/_lib.py is that binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch tensors'
 *    data_ptr()); the library never allocates, frees or synchronises;
 *  - activations are fp32 NHWC ("[N,H,W,C]") unless stated; tensors at the
 *    drop-in boundary (network input, heatmaps, targets) are NCHW;
 *  - `stream` is a hipStream_t; every call only enqueues kernels on it and is
 *    therefore hipGraph-capturable;
 *  - `accumulate`/`acc_*` = 0: overwrite the output, 1: add into it;
 *  - returns 0, or FAMI_EARG (-1) bad argument, FAMI_ESHAPE (-2) unsupported
 *    shape, FAMI_EHIP (-3) HIP error; fami_last_error() has the text
 *    (thread-local);
 *  - workspaces: size from the matching fami_*_workspace() query (bytes).
 */
#ifndef FAMI_H
#define FAMI_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* fami_stream_t; /* hipStream_t */

/* ---- routing state: which kernel form an entry point dispatches to ---------------------------------------------------
 * "no global mutable state besides a kernel cache => re-entrant per stream".  Every such switch is a NAMED FIELD
 * of fami_route_t (fami_route.h documents each: default, meaning, the measurement behind it).  A caller that wants routes of its
 * own (the Python Engine does) keeps a fami_route_t, initialises it with fami_route_init -- library defaults, f32 arithmetic as
 * the process default has it -- edits fields, and binds it to its thread with fami_route_bind before enqueueing work; the
 * binding is thread-local, so engines with different routes interleave in one process and threads do not see each other's.
 * With nothing bound, entry points use the process default route.  The fami_*_tune* / fami_tune_reset functions further down
 * are SHIMS kept for tests and benchmarks: they write the corresponding fields of whichever route the calling thread has bound
 * (or of the process default); the code numbers in their comments are the shim's encoding, not the interface. */
#include "fami_route.h"
long fami_route_size(void);                 /* sizeof(fami_route_t) of this build */
int fami_route_init(fami_route_t* route);   /* library defaults */
int fami_route_bind(fami_route_t* route);   /* this thread's calls route by *route until rebound; NULL = process default */

const char* fami_version(void);
const char* fami_last_error(void);
/* info[0]=CUs, [1]=wavefront, [2]=LDS bytes/workgroup, [3]=clock kHz */
int fami_device_info(int device, int* info, char* name, int name_len);

/* ---- convolution family: nn.Conv2d fwd + autograd --------------------------------------
 * replaces every nn.Conv2d of posetimation/backbones/hrnet.py:569-629 (HRNet-W48: 293 convs),
 * posetimation/layers/basic_model.py:21-23,38-41,74-77 and basic_layer.py:18-19, and the 3x3
 * dilation-3 offset/mask predictors of posetimation/zoo/Alignment/Alignment_V15.py:79-100.
 * Weights are consumed in a fragment-packed image (mode 0 = forward, 1 = dgrad). */
/* benchmarks only: force the implicit-GEMM tile (MT x NT 16x16 tiles per wave, KS-way split-K); 0 = heuristic */
int fami_conv_tune(int mt, int nt, int ks);
int fami_conv_tune_lds(int on);          /* 1 / 0 = route eligible 3x3 stride-1 convs through the LDS-staged / direct kernels,
                                          * -1 = defaults: every storage type on the register-blocked LDS kernel (conv_t4.hip), f32 through
                                          * its split-product instance (operands split exactly into three bf16 terms, six products on the
                                          * bf16 matrix pipe, fp32 accumulation).  Benchmarks / tests: 10 / 11 register-blocked kernel off /
                                          * on; 20 / 21 its exact-f32-MFMA instance; 30 / 31 the split-product instance off / on (30 = exact
                                          * f32 MFMA kernels); 52 / 53 two / three pixel tiles per wave of it; 60 / 61 / 62 its producer-
                                          * consumer form off / one-band frames / always; 100 + bt tiles per band; 2000 + n only launches of
                                          * >= n workgroups; 102000 / 102001 CU-filling band rule off / on; 102040 / 102041 the
                                          * split-product instance's weights from the pre-split image by LDS DMA off / on */
int fami_conv_tune_wgrad_lds(int on);    /* 0 = weight gradients on the scalar-operand kernels, 1 = LDS-staged kernels wherever eligible,
                                          * 1 + n = the same with n sub-chunks per workgroup of the 16-bit kernel (default 2),
                                          * -1 = defaults (16-bit storage: LDS-staged; f32: linear-address per-tap kernel on stride-1
                                          * same-size convs, general per-tap kernel elsewhere, LDS-staged kernel opt-in);
                                          * 50 / 51 = f32 per-tap kernel in its general / linear-address form (52 / 53 / 54: the latter in
                                          * 9- / 8- / 16-wave workgroups); 100 + mt, 1000 + n = benchmarks (tile cap, workgroup target);
                                          * 20000 + x: the pipelined 16-bit kernel (conv_wg16.hip): 0 / 1 off / on, 2 / 3 3x3-stride-1 only /
                                          * every centred geometry, 100 + bt, 1000 + target; 30000 + x: the f32 split-product kernel
                                          * (conv_wgs3.hip): 0 / 1 off / on (0 = exact-f32 MFMA kernels), 100 + bt, 1000 + target */
int fami_conv_tune_xcd(int mode);      /* benchmarks: bit 0 = XCD-contiguous workgroup->tile order in the implicit-GEMM kernels,
                                        * bit 1 = in the weight-gradient kernels; -1 = default (both on) */
int fami_conv_tune_stages(int stages); /* benchmarks only: register-pipeline depth 2..4, 0 = default;
                                        * 100 / 101 = linear-address form of the f32 implicit GEMM off / on (default on);
                                        * 110 / 111 = stride-2 input gradient: all taps / the pixel's parity class only (default) */
/* Every field of the calling thread's route (bound or process default) back to its default (tests: autouse fixture).  The
 * fields only select between kernels that compute the same function. */
int fami_tune_reset(void);
/* The library's default f32 arithmetic for 3x3 stride-1 convolutions (1 = split products on the bf16 matrix pipe,
 * 0 = exact-f32 MFMA, < 0 = keep) -- stored as the default that fami_tune_reset / fami_conv_tune_lds(-1) restore --
 * then fami_tune_reset.  _lib.py calls it once at load with FAMI_F32_SPLIT. */
int fami_tune_defaults(int f32_split);
/* would a 3x3 stride-1 pad-1 f32 convolution [N,H,W,Ci] -> Co take the persistent split-product kernel (conv_t5.hip)? (tests) */
int fami_conv_t5_eligible(int N, int H, int W, int Ci, int Co);
/* would a 3x3 stride-1 pad-1 f32 convolution [N,H,W,Ci] -> Co take the split-product band kernel (conv_t4.hip) with the input
 * BatchNorm's tables in LDS (the f32 half of fami_conv2d_xbn_ok_f32)? (tests) */
int fami_conv_t4_eligible(int N, int H, int W, int Ci, int Co);
/* ... and which form of it would a launch be: 0 none, 1 the register form (every workgroup splits its f32 weight fragments),
 * 2 the weight-DMA form (pre-split image -> LDS by DMA, two weight buffers; fami_conv_tune_lds(102040 / 102041) off / on),
 * 3 producer / consumer.  dil: dilation = padding; sgn -1: the input gradient, with Ci / Co as that launch takes them (swapped);
 * xbn: with the input BatchNorm's tables in LDS.  out (optional, 5 longs; forms 1 and 2): LDS bytes of the register form, LDS
 * bytes the DMA form needs (it is taken only where they fit 160 KiB), 16-pixel tiles per band, pixel tiles per wave of the
 * instance (2 | 3), patch pieces per thread. (tests) */
int fami_conv_t4_s3_plan(int N, int H, int W, int Ci, int Co, int dil, int sgn, int xbn, long* out);
/* ... and the LDS-DMA-staged kernels of conv_t6.hip (round 4: 16-bit storage; 48 input channels: whole weight image LDS-resident,
 * patch and weights copied by LDS DMA -- fami_conv_tune_lds(8000 / 8001) off / on, 8100 + rows per band, 8201 / 8202 units of two /
 * four rows, 8400 + minimum jobs; 96 / 192 / 384 input channels in phases of 48 -- 8500 / 8501 off / on, 8600 + rows per band,
 * 8700 + workgroups per output-channel block)?  Returns 1 (the 48-channel kernel), 2 (the phased kernel) or 0.
 * fami_conv_tune_lds(9000 / 9001): the stem's dense-K 3 -> 64 stride-2 forward kernel (conv_stem.hip, every storage type) off / on.
 * Weight gradients: fami_conv_tune_wgrad_lds(23000 / 23001) the DMA-staged 3x3
 * kernel off / on (23002 / 23003 its 64-channel blocks, 23004 / 23005 stride 2, 23008 / 23009 the dilated 48 -> 216 / 108
 * predictors of the alignment head, 23100 + units per workgroup, 23400 + workgroup target), 24000 / 24001 the
 * DMA-staged wide 1x1 kernel off / on (24100 + workgroup target), 25000 / 25001 the stem's 3 -> 64 weight-gradient kernel. */
int fami_conv_t6_eligible(int N, int H, int W, int Ci, int Co);
long fami_packed_weight_elems(int Co, int Ci, int kh, int kw, int mode);
int fami_pack_conv_weight_f32(const float* w_oihw, float* wp, int Co, int Ci, int kh, int kw, int mode,
                              fami_stream_t stream);
/* all weight images of a step in one launch: desc = device array of n 32-byte records
 * {long src_elem_off (in params), long dst_elem_off (in packed), int Co, int Ci, int taps, int mode} */
int fami_pack_conv_weights_batch_f32(const float* params, float* packed, const void* desc, int n, fami_stream_t stream);
/* y[N,Ho,Wo,Co] (=|+=) relu?( conv(x[N,H,W,Ci]) + bias + addend ) ; bias/addend may be NULL */
int fami_conv2d_fwd_f32(const float* x, const float* wp, const float* bias, const float* addend, float* y, int N,
                        int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil, int relu,
                        int accumulate, fami_stream_t stream);
/* dx[N,H,W,Ci] (=|+=) conv_transpose(dy[N,Ho,Wo,Co]) + addend */
int fami_conv2d_dgrad_f32(const float* dy, const float* wp, const float* addend, float* dx, int N, int H, int W,
                          int Ci, int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                          fami_stream_t stream);
/* Convolution with the statistics pass of the train-mode BatchNorm that follows it (basic_model.py:34-63: every conv of
 * a block feeds nn.BatchNorm2d) folded into the epilogue: per-channel sums of (y - pivot), (y - pivot)^2 go into the fp64
 * slot rows of fami_bn_slots_bytes(Co) bytes (ZERO on entry), pivot = pivot_src[c] (the running mean; NULL = 0) is
 * stored behind the rows.  Consumers: fami_bn_apply_slots_* / fami_bn_finalize_slots_f32.
 * fami_conv2d_dgrad_bnstats_*: the input-gradient convolution that makes the LAST contribution to dx = dL/d(output of a
 * train-mode BatchNorm [+ReLU] whose input was z): stores dz = relu-mask(dx) instead of dx and adds sum dz, sum dz*xhat
 * into `slots` (fami_bn_slots_bytes(Ci), ZERO on entry) for fami_bn_bwd_apply_slots_*.  relu: 0 none, 1 mask from the
 * BatchNorm output yrelu, 2 mask recomputed from z (forward run by fami_bn_train_fwd2 / fami_bn_apply_slots). */
int fami_conv2d_fwd_stats_f32(const float* x, const float* wp, const float* bias, float* y, int N, int H, int W, int Ci,
                              int Co, int kh, int kw, int stride, int pad, int dil, void* slots, const float* pivot_src,
                              fami_stream_t stream);
int fami_conv2d_dgrad_bnstats_f32(const float* dy, const float* wp, float* dx, int N, int H, int W, int Ci, int Co,
                                  int kh, int kw, int stride, int pad, int dil, int accumulate, const float* z,
                                  const float* yrelu, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, int relu, void* slots, fami_stream_t stream);
long fami_conv2d_wgrad_workspace(int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil);
/* Deferred slab reduce (the weight-gradient kernels write per-workgroup partial slabs; the reference's autograd has no
 * counterpart): fami_conv2d_wgrad_defer_* launches the kernel and describes its reduce in desc_out -- a HOST buffer of
 * fami_wgrad_reduce_desc_longs() longs -- and fami_wgrad_reduce_batch launches up to 16 described reduces per kernel
 * launch (descs: n consecutive descriptors on the host).  Same summation order as the immediate reduce. */
int fami_wgrad_reduce_desc_longs(void);
int fami_wgrad_reduce_batch(const long* descs, int n, fami_stream_t stream);
int fami_conv2d_wgrad_defer_f32(const float* x, const float* dy, float* dw, float* workspace, long ws_bytes, int N,
                                int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                                int accumulate, long* desc_out, fami_stream_t stream);
/* dw[Co,Ci,kh,kw] (OIHW, =|+=) */
int fami_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* workspace, long ws_bytes, int N, int H,
                          int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                          fami_stream_t stream);

/* ---- BatchNorm (+ReLU, +residual) : nn.BatchNorm2d(momentum 0.1, eps 1e-5) ---------------
 * replaces basic_model.py:34,42 (BasicBlock.bn1/bn2 + `out += residual` + ReLU :46-63),
 * :75-79 (Bottleneck), basic_layer.py:25-26, hrnet.py:107,127,138 (fuse BNs).  x is [P,C]. */
long fami_bn_workspace(int C);
int fami_bn_stats_f32(const float* x, long P, int C, float* mean, float* invstd, float* running_mean,
                      float* running_var, float momentum, float eps, float* ws, fami_stream_t stream);
/* train-mode forward in one call: batch statistics (+ running-stat update) and apply (+ residual, + ReLU);
 * tensors of <= 16384 pixels (the low-resolution branches) run as ONE launch */
int fami_bn_train_fwd_f32(const float* x, const float* residual, float* y, const float* gamma, const float* beta,
                          float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,
                          int relu, float momentum, float eps, float* ws, fami_stream_t stream);
/* running_mean / running_var update from a finished (mean, invstd) of a train-mode call that was run with NULL running
 * pointers: shared BatchNorm modules can then run concurrently on several streams and be updated afterwards in call
 * order (var = 1/invstd^2 - eps, unbiased for running_var as nn.BatchNorm2d) */
int fami_bn_running_update_f32(float* running_mean, float* running_var, const float* mean, const float* invstd, int C,
                               long P, float momentum, float eps, fami_stream_t stream);
/* n deferred updates in call order, one launch per 32: ptrs = host array of 4 n longs (running_mean, running_var, mean,
 * invstd), meta = host array of 4 n floats (C, P, momentum, eps) */
int fami_bn_running_update_batch_f32(const long* ptrs, const float* meta, int n, fami_stream_t stream);
int fami_bn_eval_stats_f32(const float* running_mean, const float* running_var, float* mean, float* invstd, int C,
                           float eps, fami_stream_t stream);
int fami_bn_apply_f32(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* residual, float* y, long P, int C, int relu, fami_stream_t stream);
int fami_bn_bwd_f32(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                    const float* gamma, float* dx, float* dgamma, float* dbeta, float* dres, long P, int C, int relu,
                    int acc_dx, int acc_param, int acc_dres, float* ws, fami_stream_t stream);
/* Backward with FROZEN statistics (eval-mode BatchNorm: mean / invstd are constants): dz = relu ? dy*(y>0) : dy;
 * dx (=|+=) dz*gamma*invstd; dres (=|+=) dz; dbeta (=|+=) sum dz; dgamma (=|+=) sum dz*(x-mean)*invstd.  One data pass,
 * plus a channel-sized fixed-order fp64 finalize when dgamma / dbeta are given (ws: fami_bn_workspace(C)); run-to-run
 * bitwise.  dgamma and dbeta both NULL: no sums, one launch, x / mean / ws are not read. */
int fami_bn_eval_bwd_f32(const float* dy, const float* x, const float* y, const float* mean,
                     const float* invstd, const float* gamma, float* dx, float* dgamma, float* dbeta,
                     float* dres, long P, int C, int relu, int acc_dx, int acc_param, int acc_dres, float* ws,
                     fami_stream_t stream);
/* Two-launch forms of the two calls above (fami_bn_{stats,finalize,apply,bwd}; the finalize launch is folded
 * into the apply pass): the statistics pass adds its partial sums into fp64 slot rows, every workgroup of the apply pass
 * folds them in its prologue.  `slots`: fami_bn_slots_bytes(C) bytes, ZERO on entry (the caller clears one arena per
 * step).  Backward relu: 0 none, 1 mask from y, 2 mask recomputed from x (no residual; y may be NULL) -- the latter only
 * against a forward run by fami_bn_train_fwd2 (same fused multiply-add of scale / shift).  Sums arrive in atomic order:
 * reproducible to fp64 rounding, not bit for bit -- the three-launch forms stay for the deterministic mode. */
long fami_bn_slots_bytes(int C);
int fami_bn_train_fwd2_f32(const float* x, const float* residual, float* y, const float* gamma, const float* beta,
                           float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,
                           int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd2_f32(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, float* dres, long P,
                     int C, int relu, int acc_dx, int acc_param, int acc_dres, void* slots, fami_stream_t stream);
/* The apply passes alone, for slot rows a convolution epilogue has filled (fami_conv2d_fwd_stats_* /
 * fami_conv2d_dgrad_bnstats_*): one launch per BatchNorm pass instead of two.  dz: the gradient with the ReLU mask
 * already applied.  fami_bn_is_small: tensors the one-launch small-tensor kernel takes (no point fusing those).
 * fami_bn_finalize_slots_f32: mean / invstd / running update only (HighResolutionModule fuse terms, hrnet.py:151-172). */
int fami_bn_is_small(long P, int C);
/* conv1 -> BatchNorm -> ReLU -> conv2 without the normalised tensor in HBM (16-bit modes; basic_model.py:34-63): conv2's
 * forward (fami_conv2d_fwd_xbn_*) and weight gradient (fami_conv2d_wgrad_defer_xbn_*) take the PRE-normalisation tensor z
 * and apply scale / shift / ReLU while they stage it into LDS.  fami_conv2d_xbn_ok: can a 3x3 stride-1 pad-1 convolution of
 * this shape do that (both kernels eligible)? */
int fami_conv2d_xbn_ok(int N, int H, int W, int Ci, int Co);
/* Round 6: the train-mode BatchNorm + ReLU in front of a 3x3 stride-1 convolution INSIDE that convolution's launch, with the
 * normalised tensor written out as well (a_out [N,H,W,Ci]: what the reference materialises between conv1 and conv2 of a BasicBlock,
 * basic_model.py:34-63; the backward pass reads it).  z = the BatchNorm's input, xslots = its statistics rows (filled by
 * fami_conv2d_fwd_stats_* of the producing convolution); mean / invstd / running statistics are published as by
 * fami_bn_apply_slots_*.  Results bit for bit those of fami_bn_apply_slots_* followed by fami_conv2d_fwd(_stats)_*. */
int fami_conv2d_fwd_bnin_ok(int N, int H, int W, int Ci, int Co);
/* Backward of a 3x3 stride-1 pad-1 convolution as ONE launch (16-bit modes; nn.Conv2d autograd of basic_model.py:44-63):
 * the input gradient (fami_conv2d_dgrad_* / fami_conv2d_dgrad_bnstats_* when slots != NULL) and the deferred weight gradient
 * (fami_conv2d_wgrad_defer_*) read the same dY and nothing of each other; fami_conv2d_bwd_pair_* runs the two kernels' bodies
 * side by side in one grid (weight-gradient workgroups first).  Bitwise the two-call form; where no combined instance exists
 * the two single launches run.  fami_conv2d_bwd_pair_ok: does a combined instance take this geometry (forward geometry)?
 * fami_conv2d_bwd_pair_key: the kernel instances of the two halves (tools / tests; out[9]). */
int fami_conv2d_bwd_pair_ok(int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil);
int fami_conv2d_bwd_pair_key(int N, int H, int W, int Ci, int Co, int* out);
/* f32 storage: the split-product input gradient and the deferred split-product weight gradient of a 3x3 stride-1 convolution in one
 * launch (xmean != NULL: x is the input z of a BatchNorm + ReLU nobody materialised, as fami_conv2d_wgrad_defer_xbn_f32). */
int fami_conv2d_bwd_pair_ok_f32(int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil);
int fami_conv2d_bwd_pair_key_f32(int N, int H, int W, int Ci, int Co, int* out);
int fami_conv2d_bwd_pair_f32(const float* x, const float* dy, const float* wpd, float* dx, float* dw, float* workspace,
                             long ws_bytes, int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                             int acc_dx, int acc_dw, long* desc_out, const float* xmean, const float* xinvstd,
                             const float* xgamma, const float* xbeta, fami_stream_t stream);
/* the same in f32 storage (the split-product kernels; FAMI_XBN=1) */
int fami_conv2d_xbn_ok_f32(int N, int H, int W, int Ci, int Co);
int fami_conv2d_fwd_xbn_f32(const float* z, const float* wp, const float* bias, float* y, int N, int H, int W, int Ci,
                            int Co, void* slots, const float* pivot_src, const void* xslots, long xP,
                            const float* xgamma, const float* xbeta, float* xmean, float* xinvstd,
                            float* xrunning_mean, float* xrunning_var, float xmomentum, float xeps, fami_stream_t stream);
int fami_conv2d_wgrad_defer_xbn_f32(const float* z, const float* dy, float* dw, float* workspace, long ws_bytes, int N,
                                    int H, int W, int Ci, int Co, int accumulate, long* desc_out, const float* xmean,
                                    const float* xinvstd, const float* xgamma, const float* xbeta, fami_stream_t stream);
/* benchmarks: element count up to which a tensor takes the one-launch small-tensor kernels (< 0: default 32768) */
int fami_bn_tune_small(long elems);
int fami_bn_apply_slots_f32(const float* x, const float* residual, float* y, const float* gamma, const float* beta,
                            float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,
                            int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd_apply_slots_f32(const float* dz, const float* x, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                                float* dres, long P, int C, int acc_dx, int acc_param, int acc_dres, void* slots,
                                fami_stream_t stream);
int fami_bn_finalize_slots_f32(void* slots, long P, int C, float* mean, float* invstd, float* running_mean,
                               float* running_var, float momentum, float eps, fami_stream_t stream);
long fami_channel_sum_workspace(int C);
/* out[c] (=|+=) sum_p x[p][c] : bias gradients of the biased convs */
int fami_channel_sum_f32(const float* x, long P, int C, float* out, int accumulate, float* ws, fami_stream_t stream);

/* ---- streaming helpers ---------------------------------------------------------------------
 * boundary layout converts, torch.cat/chunk (Alignment_V15.py:117-125,139,143,160), `sup - kf`
 * (:132), HighResolutionModule fuse sum + Interpolate(nearest) + ReLU (hrnet.py:159-168,
 * basic_model.py:116-125), torch.optim.Adam (posetimation/optimizer/optimizer.py:66-68). */
int fami_nchw_to_nhwc_f32(const float* src, float* dst, int N, int C, int H, int W, fami_stream_t stream);
int fami_nhwc_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W, int accumulate,
                          fami_stream_t stream);
int fami_pack_frames_f32(const float* kf_nchw, const float* sup_nchw, float* frames_nhwc, int B, int S, int H, int W,
                         fami_stream_t stream);
int fami_copy_channels_f32(const float* src, float* dst, long P, int Cs, int src_off, int Cd, int dst_off, int Cc,
                           int accumulate, fami_stream_t stream);
/* torch.cat on channels of n <= 4 tensors in one launch (c[k] % 4 == 0) and its backward: the k-th channel slice of src (=|+=) into
 * dst[k] (null: skipped).  src / dst / c / accumulate are HOST arrays of length n. */
int fami_concat_channels_f32(const float* const* src, const int* c, int n, float* dst, long P, fami_stream_t stream);
int fami_split_channels_f32(const float* src, float* const* dst, const int* c, const int* accumulate, int n, long P,
                             fami_stream_t stream);
int fami_axpby_f32(const float* a, const float* b, float* out, long n, float alpha, float beta,
                   fami_stream_t stream);
int fami_fill_f32(float* out, long n, float v, fami_stream_t stream);
/* dst (=|+=) src : fp32 accumulation buffer folded into an activation-typed gradient */
int fami_cast_add_f32(const float* src, float* dst, long n, int accumulate, fami_stream_t stream);
/* dst[i] = (float)src[i] (fami_widen_bf16 / _f16: the 16-bit gradient payload of the data-parallel all-reduce widened
 * back into the fp32 gradient arena; the _f32 instance is a copy) */
int fami_widen_f32(const float* src, float* dst, long n, fami_stream_t stream);
/* out[i] (=|+=) in[i] * (sx, sy) over n (x, y) pairs: legacy kornia.warp_affine translation scaling and its gradient
 * (kornia <= 0.4 default align_corners=False at Alignment_V15.py:135: a shift of t pixels samples at x - t*W/(W-1)). */
int fami_scale_pairs_f32(const float* in, float* out, long n, float sx, float sy, int accumulate, fami_stream_t stream);
int fami_incr_i64(long long* v, long n, fami_stream_t stream);
/* v[i] += inc[i] : BatchNorm num_batches_tracked counters, all layers in one launch */
int fami_add_i64(long long* v, const long long* inc, long n, fami_stream_t stream);
/* fuse_sum and pool_relu_bwd (all three storage types) refuse non-positive N, H, W with -1 */
int fami_fuse_sum_f32(int nterms, const float* const* x, const float* const* mean, const float* const* invstd,
                      const float* const* gamma, const float* const* beta, const int* shift, float* y, int N, int H,
                      int W, int C, int relu, fami_stream_t stream);
int fami_relu_bwd_f32(const float* dy, const float* y, float* dx, long n, int accumulate, fami_stream_t stream);
int fami_pool_relu_bwd_f32(const float* dy, const float* y, float* out, int N, int Hl, int Wl, int C, int shift,
                           int relu, fami_stream_t stream);
/* out_k += a_k for n pairs of fp32 tensors in one launch per 32 pairs (the engine's lane join: lane-private gradients of a
 * module that ran on several stream lanes).  ptrs: host array of 2 n longs (a_0, out_0, a_1, out_1, ...), counts: n ints.
 * The same `out` may appear several times, and a pair's source may be an earlier pair's `out`: either starts a new launch, so
 * the adds happen in call order. */
int fami_add_batch_f32(const long* ptrs, const int* counts, int n, fami_stream_t stream);
int fami_adam_prep_f32(float* state4, float beta1, float beta2, fami_stream_t stream);
int fami_adam_f32(float* p, const float* g, float* m, float* v, long n, const float* state4, float beta1,
                  float beta2, float eps, float weight_decay, fami_stream_t stream);
/* fp16 static loss scaling with an overflow guard (the reference trains in fp32 and has no counterpart; BASELINE config 5):
 * fami_unscale_check_f32 multiplies the gradient arena by f and raises *flag (device u32) on any inf / NaN;
 * fami_adam_prep_checked_f32 then skips the whole Adam step (no step count, no moment update), clears the flag and
 * counts the skip: flag is a device u32[2] = {raised, skipped steps so far}. */
int fami_unscale_check_f32(float* g, long n, float f, unsigned* flag, fami_stream_t stream);
int fami_adam_prep_checked_f32(float* state4, float beta1, float beta2, unsigned* flag, fami_stream_t stream);
/* torch.optim.SGD (posetimation/optimizer/optimizer.py:58-64) over a flat fp32 arena.  state3 (device float[3]) =
 * {step, lr, apply}: prep increments step; the checked prep skips the step like fami_adam_prep_checked_f32 (apply = 0).
 * d = g + wd p; with momentum: buf = d on step 1, else momentum buf + (1 - dampening) d; d = nesterov ? d + momentum buf
 * : buf; p -= lr d.  buf may be NULL when momentum == 0.  Any 4-byte aligned sub-range of an arena is accepted. */
int fami_sgd_prep_f32(float* state3, fami_stream_t stream);
int fami_sgd_prep_checked_f32(float* state3, unsigned* flag, fami_stream_t stream);
int fami_sgd_f32(float* p, const float* g, float* buf, long n, const float* state3, float momentum, float dampening,
                 float weight_decay, int nesterov, fami_stream_t stream);
/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) and dynamic loss scaling
 * (torch.amp.GradScaler), device-resident: no host sync, no re-capture of a hipGraph when the threshold or the scale moves.
 * fami_sumsq_f32: the sum of squares of g[0..n) as fami_sumsq_parts() fp32 partial sums (every slot is written; one
 *   fixed contiguous chunk per workgroup, no atomics: bitwise reproducible for a given (g, n, alignment of g)).
 * fami_unscale_check_sumsq_f32: fami_unscale_check_f32 -- g *= f * (fdev ? fdev[0] : 1), *flag raised on inf / NaN --
 *   that also leaves the sum of squares of the unscaled values in partials (may be NULL).
 * fami_accum_unscale_check_sumsq_f32: the pass that closes a gradient-accumulation window, g[i] = rn(rn(acc[i] + g[i]) * mul)
 *   with mul formed as above; acc is only read; flag (may be NULL: no check) is raised on inf / NaN in what was written;
 *   partials (may be NULL) is bit for bit what fami_sumsq_f32 returns on the g this pass leaves.  One launch instead of
 *   fami_axpby_f32(acc, g, g, 1, 1) + fami_unscale_check_sumsq_f32, with the same result in the arena, the slab and the flag.
 * fami_clip_coef_f32: clip (device float[2]) = {total_norm, coef}; the partials are summed in double in a fixed order,
 *   coef = min(1, max_norm_dev[0] / (total_norm + 1e-6f)).  A non-finite norm raises flag[0] (coef = 0), so the checked
 *   prep kernels skip and count the step like an fp16 overflow.  That differs from torch on purpose: clip_grad_norm_'s
 *   default error_if_nonfinite=False lets a NaN norm through into every parameter.
 * fami_adam_scaled_f32 / fami_sgd_scaled_f32: fami_adam_f32 / fami_sgd_f32 with the gradient gmul[0] * g on load (gmul:
 *   device float, e.g. clip + 1); the gradient arena is not rewritten; gmul[0] == 1 gives the unscaled result bit for bit.
 * fami_loss_scale_update_f32: scaler (device float[3]) = {scale, 1 / scale, growth tracker}; flag[0] raised: scale *=
 *   backoff, tracker = 0; otherwise tracker += 1 and at `interval`: scale *= growth (refused when that is inf), tracker =
 *   0.  It only reads the flag: enqueue it before the checked prep that clears it. */
int fami_sumsq_parts(void);
int fami_sumsq_f32(const float* g, long n, float* partials, fami_stream_t stream);
int fami_unscale_check_sumsq_f32(float* g, long n, float f, const float* fdev, unsigned* flag, float* partials,
                                 fami_stream_t stream);
int fami_accum_unscale_check_sumsq_f32(float* g, const float* acc, long n, float f, const float* fdev, unsigned* flag,
                                       float* partials, fami_stream_t stream);
int fami_clip_coef_f32(const float* partials, int nparts, const float* max_norm_dev, float* clip, unsigned* flag,
                       fami_stream_t stream);
int fami_adam_scaled_f32(float* p, const float* g, float* m, float* v, long n, const float* state4, float beta1,
                         float beta2, float eps, float weight_decay, const float* gmul, fami_stream_t stream);
int fami_sgd_scaled_f32(float* p, const float* g, float* buf, long n, const float* state3, float momentum,
                        float dampening, float weight_decay, int nesterov, const float* gmul, fami_stream_t stream);
int fami_loss_scale_update_f32(float* scaler, const unsigned* flag, float growth, float backoff, int interval,
                               fami_stream_t stream);
/* Exponential moving average (EMA) of a flat fp32 parameter arena, device-resident: no host sync, and a captured hipGraph
 * keeps replaying while steps are applied or skipped.
 * fami_ema_prep_f32: one thread.  st4 (device float[4]) = {updates, decay_t, w, apply}.  gate (device float, may be NULL):
 *   the optimizer's "this step was applied" scalar -- state[2] of fami_adam_prep_* / fami_sgd_prep_*.  gate[0] == 0:
 *   apply = 0 and nothing else changes.  Otherwise t = updates + 1, updates = t, decay_t = warmup ? min(decay,
 *   (1 + t) / (10 + t)) : decay, w = 1 - decay_t (one fp32 subtraction), apply = 1.  decay must lie in (0, 1).
 * fami_ema_update_f32: returns at once when st4[3] == 0; otherwise ema[i] = rn(ema[i] + rn(w * rn(p[i] - ema[i]))) with
 *   w = st4[2] -- three separately rounded fp32 operations, no fused multiply-add.  p is only read.  12 bytes of traffic
 *   per element.
 * fami_swap_f32: exchanges the contents of a and b bit for bit in one pass, with no temporary.
 * Both passes accept any 4-byte aligned sub-ranges of arenas; the two arrays must not overlap. */
int fami_ema_prep_f32(float* st4, const float* gate, float decay, int warmup, fami_stream_t stream);
int fami_ema_update_f32(float* ema, const float* p, long n, const float* st4, fami_stream_t stream);
int fami_swap_f32(float* a, float* b, long n, fami_stream_t stream);

/* ---- temporal alignment ----------------------------------------------------------------------
 * fami_shift_bilinear_*: kornia.geometry.warp_affine(src, [[1,0,tx],[0,1,ty]], dsize) at
 *   Alignment_V15.py:133-135 (differentiable wrt src and (tx,ty)); t is a device [B,2] = (tx,ty).
 * fami_dcn_*: torchvision.ops.DeformConv2d(C,C,3,padding=3,dilation=3).forward(x, offset, mask)
 *   at Alignment_V15.py:146,150,154,158 and its autograd; offset [B,Ho,Wo,2*G*K] ordered
 *   (group, tap, (dy,dx)), mask [B,Ho,Wo,G*K] raw (no sigmoid), G = offset groups (12). */
long fami_shift_workspace(int B);
int fami_shift_bilinear_fwd_f32(const float* src, const float* t, float* out, int B, int H, int W, int C,
                                fami_stream_t stream);
int fami_shift_bilinear_bwd_f32(const float* gout, const float* src, const float* t, float* gsrc, float* gt, int B,
                                int H, int W, int C, int acc_src, int acc_t, float* ws, fami_stream_t stream);
long fami_dcn_packed_weight_elems(int Co, int C, int kh, int kw, int G);
int fami_dcn_pack_weight_f32(const float* w_oihw, float* wp, int Co, int C, int kh, int kw, int G,
                             fami_stream_t stream);
/* the same plus the 16-bit image the bf16 / fp16 forward contracts with on the 16x16x32 matrix-core instruction (the gather's
 * vector arithmetic then overlaps the contraction); wp: fami_dcn_packed_weight_elems floats in every case */
int fami_dcn_pack_weight_bf16(const float* w_oihw, float* wp, int Co, int C, int kh, int kw, int G,
                              fami_stream_t stream);
int fami_dcn_pack_weight_f16(const float* w_oihw, float* wp, int Co, int C, int kh, int kw, int G,
                             fami_stream_t stream);
int fami_dcn_fwd_f32(const float* x, const float* off, const float* msk, const float* wp, const float* bias, float* y,
                     int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil,
                     fami_stream_t stream);
/* Benchmarks / tests: one integer code per call, each writing one align.hip field of the route bound to the calling thread
 * (include/fami_route.h).  Always returns 0.
 *   any negative  every DCN field back to its default
 *   0 / 1 / 2     dcn_gather: forward on dcn_fwd_kernel (LDS column tile) / dcn_fwd_direct_kernel (samples fed to the MFMA from
 *                 registers; the default below 4 GiB) / dcn_fwd_win_kernel (LDS window) where eligible, else the direct kernel
 *   16 + n        dcn_pf: n = 2 the direct kernel built for 2 k groups in flight x 4 waves per SIMD, n = 0 the default build
 *   32 + r        dcn_win_r: force the window kernel's offset reach to r pixels (0 = the largest that fits, up to 4)
 *   64 + bits     dcn_abl: ablation bits of the window kernel (1 no MFMA, 2 no LDS gather, 4 no offset stream, 8 no window
 *                 fill, 16 constant weights, 32 no loop; f32 with Co in 33..48 only)
 *   256 + k       dcn_ksplit: k = 2 the 16-wave K-split build of the window kernel, k = 1 the default 8-wave build
 *   512 + m       dcn_bwd_scatter, the backward's input-gradient scatter: m = 0 f32 compare-and-swap LDS region, 1 fixed-point
 *                 region (64-bit for f32, 32-bit for 16-bit storage; the default), 2 64-bit region for every type.  Only the
 *                 default runs on the register-fed backward kernel; the others select the general kernel
 *   1024 + bits   dcn_bwd_abl: ablations of the general backward kernel (1 no region flush, 2 no LDS adds, 4 constant scale)
 *   2048 + n      dcn_bwd2: the register-fed backward kernel off (n = 0) / on (n = 1, default)
 *   4096 + KB     dcn_bwd2_cap: LDS budget of the register-fed kernel's region (default 36; decides the groups per workgroup
 *                 and with them the weight image: set BEFORE fami_dcn_pack_weight_bwd_f32)
 *   8192 + n      dcn_bwd2_stage: offset / mask gradients of the register-fed kernel staged in LDS off (0) / on (1, default) */
int fami_dcn_tune(int mode);
long fami_dcn_packed_weight_bwd_elems(int Co, int C, int kh, int kw, int G);
int fami_dcn_pack_weight_bwd_f32(const float* w_oihw, float* wpb, int Co, int C, int kh, int kw, int G,
                                 fami_stream_t stream);
/* Column count of the `col` matrix the fami_dcn_bwd_* / fami_dcn_bwd_om_* entry points write for this geometry and storage
 * size (elem_bytes 4 | 2): C*kh*kw in weight.view(Co, C*K) order on the general kernel (always in the deterministic form), or
 * more -- the register-fed kernel writes the modulated samples in its own (chunk, tap, group, channel) column order, padded to
 * whole 16-column blocks (fami_dcn_bwd_col_permuted says which; the widths can coincide).  In that case the caller's 1x1 weight
 * gradient over col is [Co][cols], and
 * fami_dcn_col_dw_unpermute_f32 (=|+=) brings it into the OIHW order of DeformConv2d.weight (Alignment_V15.py:83-101). */
long fami_dcn_bwd_col_width(int C, int Co, int G, int kh, int kw, int stride, int dil, int elem_bytes, int deterministic);
int fami_dcn_bwd_col_permuted(int C, int Co, int G, int kh, int kw, int stride, int dil, int elem_bytes, int deterministic);
int fami_dcn_col_dw_unpermute_f32(const float* dwp, float* dw, int Co, int C, int G, int kh, int kw, int stride, int dil,
                                  int elem_bytes, int accumulate, fami_stream_t stream);
/* autograd of DeformConv2d wrt input / offsets / masks (fused: column gradient dy x W stays in LDS).
 * col [P, C*K] (out, may be NULL) = modulated samples, column order (channel, tap) == weight.view(Co, C*K):
 * dW[co, kidx] = sum_p dy[p,co] * col[p,kidx], the caller runs that GEMM (fami_conv2d_wgrad_f32, 1x1).
 * gx [B,H,W,C] is ACCUMULATED with atomics (zero it first); goff/gmsk (=|+=) per acc_off; each may be NULL. */
int fami_dcn_bwd_f32(const float* x, const float* off, const float* msk, const float* dy, const float* wpb,
                     float* col, float* gx, float* goff, float* gmsk, int B, int H, int W, int C, int Co, int G,
                     int kh, int kw, int stride, int pad, int dil, int acc_off, fami_stream_t stream);

/* Run-to-run deterministic form of fami_dcn_bwd_f32 ("an fp32 deterministic path for the parity config"):
 * the scatter of the input gradient adds 64-bit fixed-point integers (associative, so independent of arrival order)
 * scaled by 2^(42 - ceil(log2 max|dy|)); gx [B,H,W,C] is then written (=|+= per acc_x) by a conversion pass.
 * Overflow needs one input element to collect more than 2^20 x max|dy|.  ws: fami_dcn_bwd_det_workspace bytes. */
long fami_dcn_bwd_det_workspace(int B, int H, int W, int C);
int fami_dcn_bwd_det_f32(const float* x, const float* off, const float* msk, const float* dy, const float* wpb,
                         float* col, float* gx, float* goff, float* gmsk, int B, int H, int W, int C, int Co, int G,
                         int kh, int kw, int stride, int pad, int dil, int acc_off, int acc_x, void* ws,
                         fami_stream_t stream);

/* The three DCN entry points above for offsets and masks held in ONE tensor om [B,Ho,Wo,3GK] -- per pixel the 2GK offsets
 * followed by the GK masks: what the offset and the mask predictor of a DCN layer (Alignment_V15.py:79-100, called at
 * :144-158) produce when they run as one 48 -> 324 convolution (weights concatenated on the output-channel axis; the
 * state_dict keeps the two modules).  gom: the gradient wrt om, same layout (=|+= per acc_om).  Same kernels, other strides. */
int fami_dcn_fwd_om_f32(const float* x, const float* om, const float* wp, const float* bias, float* y, int B, int H, int W,
                       int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, fami_stream_t stream);
int fami_dcn_bwd_om_f32(const float* x, const float* om, const float* dy, const float* wpb, float* col, float* gx, float* gom,
                       int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, int acc_om,
                       fami_stream_t stream);
int fami_dcn_bwd_det_om_f32(const float* x, const float* om, const float* dy, const float* wpb, float* col, float* gx,
                           float* gom, int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad,
                           int dil, int acc_om, int acc_x, void* ws, fami_stream_t stream);

/* ---- dense layers of the translation regressor: nn.Linear x3 (Alignment_V15.py:69-71) ------- */
int fami_linear_fwd_f32(const float* x, const float* w, const float* b, float* y, int M, int K, int N,
                        fami_stream_t stream);
/* dx, dw, db may be null, except db without dw (-1: the bias gradient comes from the launch of dw) */
int fami_linear_bwd_f32(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int M,
                        int K, int N, int acc_dx, int acc_param, fami_stream_t stream);

/* ---- targets / losses / decode (NCHW rows) ----------------------------------------------------
 * fami_gauss_target : datasets/process/heatmaps_process.py:146-203 (generate_heatmaps)
 * fami_wmse_*       : posetimation/loss/mse_loss.py:21-40 (JointMSELoss.forward)
 * fami_softmax_kl_* : Alignment_V15.py:250-277 (feat_label/feat_feat MI estimators, T = 0.05)
 * fami_argmax2d      : datasets/process/heatmaps_process.py:16-44 (get_max_preds) */
int fami_gauss_target_f32(const float* joints_xy, const float* vis, float* target, float* weight, int B, int J,
                          int Hh, int Wh, int img_h, int img_w, int sigma, fami_stream_t stream);
/* joint_w: DEVICE float[J] or NULL (weight[b,j] *= joint_w[j]); subpixel != 0: Gaussian centred at the real-valued joint
 * position inside the rounded centre's window.  (NULL, 0) writes what fami_gauss_target_f32 writes. */
int fami_gauss_target_ex_f32(const float* joints_xy, const float* vis, const float* joint_w, float* target,
                             float* weight, int B, int J, int Hh, int Wh, int img_h, int img_w, int sigma, int subpixel,
                             fami_stream_t stream);
int fami_wmse_fwd_f32(const float* pred, const float* gt, const float* w, float* loss, int R, int L, double scale,
                      float* ws, fami_stream_t stream);
/* online hard keypoint mining: per sample the k joints with the largest row sums (ties: lower index; NaN first);
 * sel_w [B*J] = w (1 if NULL) where selected, else 0; loss = scale * their sum (fp64, fixed order); ws: B*J floats;
 * 1 <= k <= J or -1.  Gradient: fami_wmse_bwd_f32 with sel_w as w. */
int fami_ohkm_fwd_f32(const float* pred, const float* gt, const float* w, float* loss, float* sel_w, int B, int J, int L,
                      int k, double scale, float* ws, fami_stream_t stream);
int fami_wmse_bwd_f32(const float* pred, const float* gt, const float* w, float* dpred, int R, int L, float scale,
                      const float* gdev, int accumulate, fami_stream_t stream);
int fami_softmax_kl_fwd_f32(const float* A, const float* Bt, float* value, float* stats, int R, int L,
                            float temperature, float* ws, fami_stream_t stream);
int fami_softmax_kl_bwd_f32(const float* A, const float* Bt, const float* stats, float* dBt, int R, int L,
                            float temperature, float gscale, const float* gdev, int accumulate,
                            fami_stream_t stream);
/* idx[r]: the first maximum of row r; NaN as in numpy (np.argmax / np.amax): the first NaN of the row, maxval NaN.
 * fami_final_preds_f32 and fami_pck_accuracy_f32 then zero such a joint through their `maxval > 0` tests. */
int fami_argmax2d_f32(const float* hm, long long* idx, float* maxval, int R, int L, fami_stream_t stream);
/* get_final_preds (datasets/process/heatmaps_process.py:47-73 + transform_preds, affine_transform.py:13-43, rot 0):
 * argmax, quarter-pixel shift, inverse affine to image coordinates.  hm [B,J,H,W]; center, scale [B,2];
 * preds [B,J,2]; maxvals [B,J]; idx_ws: B*J int64 scratch */
int fami_final_preds_f32(const float* hm, const float* center, const float* scale, float* preds, float* maxvals,
                         long long* idx_ws, int B, int J, int H, int W, fami_stream_t stream);
/* dark_get_final_preds (datasets/process/heatmaps_process.py:84-143; csrc/decode.hip): the distribution-aware decode.
 * Per map, in fp32 and in this order: get_max_preds on the unblurred map (maxvals and the integer coordinates are those
 * of fami_final_preds_f32 bit for bit); a k x k separable Gaussian blur with zero padding, rescaled by
 * origin_max / max(blurred); log(max(., 1e-10)); one Newton step from the 5-point gradient and Hessian at the integer
 * peak where 1 < px < W-2, 1 < py < H-2 and the determinant is not 0; transform_preds for rot 0.  Where the rescale
 * ratio is not finite (blurred maximum exactly 0; NaN coordinates in the reference) the step is skipped.
 * hm [B,J,H,W]; center, scale [B,2]; taps: DEVICE float[k], the fp64 kernel exp(-x^2 / (2 sigma^2)) normalised to sum 1
 * and rounded to fp32 (OpenCV: sigma = 0.3 ((k-1)/2 - 1) + 0.8; symmetric: only taps[0 .. (k-1)/2] are read and each
 * mirror pair of samples is added before it is scaled), k odd with 9 <= k <= 17 (else -1); preds [B,J,2];
 * maxvals [B,J].  One launch, one workgroup per map, no workspace and no host read-back.  The map and its row pass live
 * in LDS: fami_dark_preds_lds_bytes(H, W, k) = 4 (H (W + k - 1) + (H + k - 1) W) bytes (-1 for a k or size that is no
 * argument) must not exceed fami_dark_preds_lds_limit(), else -2 before any launch (128x96 at k = 17: 112640 of
 * 163584).  Any W: no alignment is assumed. */
int fami_dark_preds_f32(const float* hm, const float* center, const float* scale, const float* taps, int k, float* preds,
                        float* maxvals, int B, int J, int H, int W, fami_stream_t stream);
long fami_dark_preds_lds_bytes(int H, int W, int k);
long fami_dark_preds_lds_limit(void);

/* ---- integral (soft-argmax) coordinates: loss term and decode (csrc/loss.hip) -------------------
 * Integral pose regression (Sun et al., ECCV 2018): an L1 loss on the soft-argmax of the heatmap -- the term the
 * reference's train loop constructs (alignment_mi_function_term6_1.py:61-69, LOSS.INTEGRAL_L1.USE / .WEIGHT) from a file
 * that was never released.  This project's definition; beta = 1 / T with the reference's heatmap temperature T = 0.05.
 * Row: one heatmap hm[b, j] of H x W fp32 values h_i at pixel (x_i, y_i), x in 0..W-1, y in 0..H-1.
 * Forward: a_i = beta * h_i (ONE fp32 rounding, never contracted), m = max a_i, e_i = expf(a_i - m), Z = sum e_i,
 *   cx = sum e_i x_i / Z, cy = sum e_i y_i / Z in heatmap pixels; coords[r] = {cx, cy}, stats[r] = {m, Z}.
 * Target position (tx, ty): the joint in heatmap pixels, joint / feature stride -- fami_heatmap_xy_f32 evaluates the
 *   expression fami_gauss_target_ex_f32(subpixel = 1) centres its Gaussian at, (double)joint / ((double)img / size), and
 *   rounds it to fp32.
 * Loss: L = scale * sum_r w_r (|cx_r - tx_r| / W + |cy_r - ty_r| / H); w [R] (the target weights; NULL: 1); the row values
 *   are summed in fp64 in a fixed order as in fami_wmse_fwd_f32 (ws: R floats).  The caller's scale is weight / (B J).
 * Backward: dhm[r,i] (=|+=) g w_r beta p_i (sgn(cx - tx) (x_i - cx) / W + sgn(cy - ty) (y_i - cy) / H) with
 *   p_i = expf(beta h_i - m) / Z recomputed from stats, sgn(0) = 0, g = scale * (gdev ? gdev[0] : 1): the
 *   fami_wmse_bwd_f32 convention.  fami_softargmax_bwd_f32 is the soft-argmax alone:
 *   dhm[r,i] (=|+=) beta p_i (gcoords[r,0] (x_i - cx) + gcoords[r,1] (y_i - cy)).
 * Decode: argmax and maxvals exactly those of fami_final_preds_f32; coordinates (cx, cy) through the same inverse affine
 *   (transform_preds, rot 0).  A joint the standard decode masks (`maxval > 0` false, NaN included) returns bit for bit
 *   what fami_final_preds_f32 returns.  One launch, no workspace, no host read-back.
 * No atomics, one 256-thread workgroup per row, the row in registers for H W <= 4096 and <= 8192 and streamed beyond, any
 * W and alignment; run-to-run bitwise reproducible.  Heatmaps are fp32 at this boundary in every compute mode.
 * beta not finite or <= 0, or a non-positive size: -1, nothing written. */
int fami_softargmax_fwd_f32(const float* hm, float* coords, float* stats, int R, int H, int W, float beta,
                            fami_stream_t stream);
int fami_softargmax_bwd_f32(const float* hm, const float* coords, const float* stats, const float* gcoords, float* dhm,
                            int R, int H, int W, float beta, int accumulate, fami_stream_t stream);
int fami_heatmap_xy_f32(const float* joints_xy, float* xy, int n, int Hh, int Wh, int img_h, int img_w,
                        fami_stream_t stream);
int fami_integral_l1_fwd_f32(const float* coords, const float* target_xy, const float* w, float* loss, int R, int H,
                             int W, double scale, float* ws, fami_stream_t stream);
int fami_integral_l1_bwd_f32(const float* hm, const float* coords, const float* stats, const float* target_xy,
                             const float* w, float* dhm, int R, int H, int W, float beta, float scale, const float* gdev,
                             int accumulate, fami_stream_t stream);
int fami_softargmax_preds_f32(const float* hm, const float* center, const float* scale, float beta, float* preds,
                              float* maxvals, int B, int J, int H, int W, fami_stream_t stream);

/* ---- structure (limb-direction cosine) loss term (csrc/loss.hip) ---------------------------------
 * The third criterion the reference's train loop constructs (alignment_mi_function_term6_1.py:60-70,
 * LOSS.STRUCTURE_COSINE.USE / .WEIGHT), again from a file that was never released: this project's definition.  It
 * supervises the DIRECTION of every limb: 1 - cosine between the predicted limb (soft-argmax coordinates) and the target limb.
 * Inputs: coords [B J, 2] fp32, the soft-argmax of the final map in heatmap pixels (fami_softargmax_fwd_f32); target_xy
 *   [B J, 2] fp32 (fami_heatmap_xy_f32); w [B J] fp32, the target weights (NULL: all 1); pairs [P, 2] int32 ON THE DEVICE:
 *   limb p goes from joint a_p to joint b_p.
 * Per sample s and limb p, in fp64 on the fp32 inputs, every operation rounded on its own (never contracted), in this order:
 *   t = txy[b] - txy[a], u = c[b] - c[a] (exact in fp64); tt = tx tx + ty ty, uu = ux ux + uy uy, ut = ux tx + uy ty;
 *   valid = w[a] > 0 && w[b] > 0 && tt > min_len^2 (a comparison with NaN is false: such a limb is not valid);
 *   nu = sqrt(uu), nt = sqrt(tt), mu = nu <= eps ? eps : nu, mt = nt <= eps ? eps : nt, cos = ut / (mu mt):
 *   torch.nn.functional.cosine_similarity's rule (with `valid` the clamp on nt is active only for min_len < eps).
 *   Row value l[s,p] = valid ? 1 - cos : 0, rounded ONCE to fp32 and stored in ws [B P].
 * Loss: L = scale * sum l, summed in fp64 in the fixed order of fami_integral_l1_fwd_f32.  The caller's scale is
 *   weight / (B P): the denominator is fixed, NOT the number of valid limbs (the integral term's convention).
 * Gradient with respect to the coordinates: nu > eps: dcos/du = t / (nu mt) - (cos u) / (nu nu); otherwise (the clamp's
 *   gradient in torch) dcos/du = t / (eps mt).  gcoords[s,j] = g sum_p valid_p (-dcos/du_p) (+1 if j == b_p, -1 if j == a_p),
 *   the limbs walked in list order, summed in fp64, the product with g rounded once to fp32; g = scale * (gdev ? gdev[0] : 1)
 *   as an fp32 product, the fami_wmse_bwd_f32 convention (a dynamic loss scale needs no host read-back).  A joint on no valid
 *   limb gets 0.  Every entry of gcoords [B J, 2] is written.  The heatmap gradient is
 *   fami_softargmax_bwd_f32(hm, coords, stats, gcoords, dhm, ..., accumulate).
 * min_len is in heatmap pixels; eps as in torch (1e-8).  1 <= P <= 64, 2 <= J <= 64.  The pair table lives on the device, so
 * the HOST checks it before upload (loss.check_structure_options: indices in 0..J-1, a != b); the kernels treat a limb that
 * breaks either rule as not valid and read nothing through it.
 * Forward: one thread per (sample, limb), then the one-workgroup fp64 sum.  Backward: one wavefront per sample, limbs then
 * joints through LDS.  No atomics, no workspace beyond ws; run-to-run bitwise reproducible.
 * A size outside the limits, min_len not finite or < 0, eps not finite or <= 0, a NULL among the required pointers (all but
 * w and gdev): -1, nothing written. */
int fami_structure_cos_fwd_f32(const float* coords, const float* target_xy, const float* w, const int* pairs, float* loss,
                               int B, int J, int P, float min_len, float eps, double scale, float* ws,
                               fami_stream_t stream);
int fami_structure_cos_bwd_f32(const float* coords, const float* target_xy, const float* w, const int* pairs,
                               float* gcoords, int B, int J, int P, float min_len, float eps, float scale,
                               const float* gdev, fami_stream_t stream);

/* PCK accuracy on heatmap argmax, engine/core/utils/evaluate.py:39-75 (`accuracy`, called twice per training step at
 * engine/core/functions/alignment_mi_function_term6_1.py:159-163 after D2H copies of four heatmap stacks): here
 * three launches and no host sync.  pred_hm / target_hm [B,J,H,W]; out[J+3] = {acc[0] = mean of the defined
 * per-joint accuracies, acc[1..J] (-1 where no valid target), avg_acc, cnt}; idx_ws 2*B*J int64, max_ws 2*B*J floats */
int fami_pck_accuracy_f32(const float* pred_hm, const float* target_hm, float* out, long long* idx_ws, float* max_ws,
                          int B, int J, int H, int W, float thr, fami_stream_t stream);

/* Flip testing (HRNet / DCPose evaluation protocol: the clip and its horizontal mirror in ONE doubled batch, the two
 * sets of heatmaps merged on the device; csrc/flip.hip).  Boundary tensors are NCHW fp32 in every compute mode.
 * fami_mirror_cat_f32: out [2*rows][W]: out[r,:] = x[r,:], out[rows+r, w] = x[r, W-1-w].  x [B,C,H,W] contiguous with
 *   rows = B*C*H gives [x ; mirror_W(x)].  A pure copy: every bit pattern survives.  x and out must not overlap.
 * fami_flip_merge_f32: hm2 [2B,J,H,W] (plain outputs, then the outputs of the mirrored inputs), perm device int[J] with
 *   every entry in [0, J): out[b,j,y,x] = (hm2[b,j,y,x] + hm2[B+b, perm[j], y, xs]) * 0.5f, xs = W-1-x, or with shift
 *   min(W-x, W-1) -- flip_back (datasets/process/pose_process.py:29-42), HRNet's flipped[..., 1:] = flipped[..., :-1]
 *   (column 0 keeps its value), then one fp32 add and one fp32 multiply.  out must not overlap hm2.
 * Both use 16-byte accesses when W % 4 == 0 and the bases are 16-byte aligned, and a scalar form for any W and any
 * 4-byte aligned pointers. */
int fami_mirror_cat_f32(const float* x, float* out, long long rows, int W, fami_stream_t stream);
int fami_flip_merge_f32(const float* hm2, const int* perm, float* out, int B, int J, int H, int W, int shift,
                        fami_stream_t stream);

/* Pose rescoring and OKS-NMS (the third step of the HRNet evaluation protocol; datasets/process/nms.py:51-192 oks_iou,
 * oks_nms, _rescore, soft_oks_nms, and the rescoring rule behind VAL/TEST.IN_VIS_THRE; csrc/nms.hip).  All pointers are
 * DEVICE memory, 4-byte aligned.  kpts [N,J,3] fp32 (x, y, confidence per joint, image pixels); area, box_score [N];
 * sigmas [J]; index [N] and seg [M+1] int: the detections of image m are index[seg[m] .. seg[m+1]) -- rows of kpts in
 * any order, at most 256 per image, an empty segment is legal.  Per image, in fp64 on the fp32 inputs:
 *   score[g] = box_score[g] * mean(conf over the joints with conf > in_vis_thre) (mean 0 when none passes), rounded to
 *     fp32 once; written for every listed detection, kept or not.
 *   The detections are then picked by descending working score (initially the fp32 score; ties: the lower position in
 *     the image's list).  OKS(picked, d) = mean over the masked joints of
 *     exp(-(dx^2 + dy^2) / (2 sigma_j)^2 / ((area_p + area_d) / 2 + 2^-52) / 2), and 0 on an empty mask.  The mask is
 *     conf_j(d) > vis_thre with use_vis != 0 -- the visibility of the COMPARED detection d only, as the reference's
 *     `list(vg > t) and list(vd > t)` evaluates -- and all joints with use_vis == 0.
 *   soft == 0 (oks_nms): a picked detection drops every remaining one with OKS > oks_thre; max_dets is not read.
 *   soft != 0 (soft_oks_nms, Gaussian): it multiplies every remaining working score by exp(-OKS^2 / oks_thre); at most
 *     max_dets are picked.  The working scores stay inside the kernel.
 *   rank[g] = position of g among its image's picks (0 = picked first), -1 = not kept; kept[m] = number picked.
 * One launch, one workgroup per image, no atomics, no workspace, no host read-back: bitwise reproducible.
 * Returns -1 before any launch for a null or misaligned pointer, J outside 1 .. 32, N outside 1 .. (2^31 - 1) / (3 J),
 * M outside 1 .. 2^31 - 2, a NaN threshold, and in soft mode oks_thre <= 0 or max_dets < 1.  index and seg are in
 * device memory and are not checked here (fami_pose_amd.evaluate.pose_nms does): an image whose segment is longer than
 * 256, is no sub-range of [0, N] or names a row outside [0, N) gets kept[m] = -1 and rank = -1 for each of its rows that
 * can be addressed (scores are still written for an over-long segment); nothing outside the three outputs is ever
 * written and other images are not affected.  A row listed twice has two writers (undefined which wins). */
int fami_pose_nms_f32(const float* kpts, const float* area, const float* box_score, const float* sigmas,
                      const int* index, const int* seg, int N, int J, int M, double in_vis_thre, double oks_thre,
                      int soft, int max_dets, double vis_thre, int use_vis, float* score, int* rank, int* kept,
                      fami_stream_t stream);

/* Pose tracking by OKS: a person identity for every listed detection (csrc/track.hip).  The reference declares
 * EVAL_TRACKING / TRACKING_THRESHOLD (posetimation/config/defaults.py:34-36) and writes track_id = position in the frame;
 * it has no association rule, so THE RULE IS THIS PROJECT'S.  All pointers are DEVICE memory, 4-byte aligned.  kpts
 * [N,J,3], area [N], sigmas [J] as for fami_pose_nms_f32; index [n]: rows of kpts grouped by frame, the frames grouped by
 * video; fseg [M+1]: the detections of frame m are index[fseg[m] .. fseg[m+1]) (at most 256; an empty frame is legal);
 * fnum [M]: its frame number; vseg [V+1]: the frames of video v are vseg[v] .. vseg[v+1) (an empty video is legal), their
 * frame numbers strictly ascending.  Per video, starting with no track and next_id = 0; a live track holds an id and the
 * (x, y) of its J joints, the box area and the frame number of the last detection matched to it:
 *   1. before frame f every live track with f - last_frame > max_gap is retired (max_gap = 1: consecutive frame numbers
 *      only; the gap is one of frame NUMBERS, not of positions in the table).
 *   2. the detections of f are walked in the order of index.  Detection d takes the live track q with the largest
 *        OKS(q, d) = mean over the masked joints of exp(-(dx^2 + dy^2) / (2 sigma_j)^2 / ((area_q + area_d) / 2 + 2^-52) / 2)
 *      (fp64 on the fp32 inputs, one rounding per operation, the sum in ascending j, 0 on an empty mask; the mask is
 *      conf_j(d) > vis_thre with use_vis != 0 and all joints with use_vis == 0) among the tracks not yet matched in this
 *      frame -- tracks created in this frame do not compete; equal OKS: the lowest id -- if that OKS is > oks_thre: then
 *      track[d] = the id of q, and q takes d's pose, area and frame number.  Otherwise d is new.
 *   3. the new detections of f get the ids next_id, next_id + 1, ... in the order of index and become live tracks.
 *   ntracks[v] = next_id at the end: ids start at 0 in every video and are never reused.
 * The result does not depend on the slot a track occupies inside the kernel.  track [N] is written for listed rows only
 * (the caller pre-fills what unlisted rows shall hold).  One launch, one workgroup per video, no atomics, no workspace,
 * no host read-back: bitwise reproducible.
 * Returns -1 before any launch for a null or misaligned pointer, J outside 1 .. 32, N outside 1 .. (2^31 - 1) / (3 J),
 * n < 0, M or V outside 1 .. 2^31 - 2, a NaN threshold, max_gap < 1.  The tables are in device memory and are not checked
 * here (fami_pose_amd.evaluate.pose_track does): a video whose segment is no sub-range of [0, M], or with a frame whose
 * segment is no sub-range of [0, n] or longer than 256, frame numbers that do not ascend, a row outside [0, N), or more
 * than 256 live tracks at once gets ntracks[v] = -1; it is left at the offending frame, so its rows hold either what they
 * held or an id.  Nothing outside the two outputs is ever written and other videos are not affected.  A row listed twice
 * has two writers (undefined which wins). */
int fami_pose_track_f32(const float* kpts, const float* area, const float* sigmas, const int* index, const int* fseg,
                        const int* fnum, const int* vseg, int N, int J, int n, int M, int V, double oks_thre,
                        int max_gap, double vis_thre, int use_vis, int* track, int* ntracks, fami_stream_t stream);

/* Track refinement: what follows fami_pose_track_f32 -- short gaps of a track filled, the poses filtered along the track,
 * the box scores replaced by the track's mean, short tracks pruned (csrc/track_refine.hip; the lists, the keys and the
 * pruning are host work, fami_pose_amd.evaluate.track_refine).  The reference has no tracker and no such step: THE RULE IS
 * THIS PROJECT'S, and this text is its contract.  Its defaults (max_fill 2, fill_conf 1, smooth_radius 2, smooth_sigma 1,
 * conf_thre 0, no rescoring, min_len 1) are STARTING VALUES, NOT TUNED: no PoseTrack data was available where it was built.
 *
 * Members.  The members of a track are the rows that the image lists name, with their id (>= 0), grouped by (video, id)
 *   -- videos in the order of their first key, ids ascending within a video -- and ordered by ascending frame number; an
 *   id occurs at most once per frame.  Rows that no image lists are carried through untouched.
 * Arithmetic.  fp64 on the inputs rounded to fp32; every operation is rounded on its own (nothing is contracted into a
 *   fused multiply-add) in the order written here; a result is rounded to fp32 once.  Nothing transcendental runs on the
 *   device: the Gaussian table g is built on the host.  fill_conf and g are doubles; conf_thre is an fp32 value and is
 *   compared with the fp32 confidences as such.
 * 1. Fill (max_fill >= 1).  For consecutive members a, b of a track with m = f_b - f_a - 1 missing frame numbers and
 *    1 <= m <= max_fill, every f in f_a + 1 .. f_b - 1 gets a new row: with t = (f - f_a) / (f_b - f_a), x and y of every
 *    joint and box columns 0 .. 4 are v_a + (v_b - v_a) * t; the confidence of joint j is min(c_a, c_b) * fill_conf and box
 *    column 5 is min(s_a, s_b) * fill_conf (min: a's value unless b's is smaller); the id is the track's.  The new rows get
 *    the numbers N, N + 1, ... in (video, id, frame) order.  A gap longer than max_fill is left alone.
 *    (The host refuses a fill that leaves a frame with more than 256 rows: the result stays a map fami_pose_track_f32's
 *    tables accept.)
 * 2. Smooth (smooth_radius >= 1; on the filled set).  For member i and joint j whose own confidence is > conf_thre: over the
 *    members k of the same track with |f_k - f_i| <= radius, in ascending frame order, those with c_kj > conf_thre
 *    contribute w = g[|f_k - f_i|] * c_kj:  sw += w; sx += w * x_k; sy += w * y_k;  then x' = sx / sw, y' = sy / sw.  If no
 *    member other than i contributes, or the own confidence fails the threshold, x and y are copied bit for bit.
 *    Confidences are never changed.  g[d] = exp(-d * d / (2 sigma^2)), d = 0 .. radius.  The output is a second array:
 *    neighbours always read unsmoothed values.  conf_thre >= 0, so every weight is positive and sw > 0.
 * 3. Rescore.  Box column 5 of every member becomes the mean of the scores its track has after the fill and before the
 *    rescoring: summed in frame order, divided by the count.
 * 4. Prune (min_len >= 2).  A track with fewer than min_len members after the fill is dropped: its rows leave the image
 *    lists (the images stay, possibly with an empty list) and hold id -1, as every row that no image lists.
 *
 * All pointers are DEVICE memory, 4-byte aligned (gauss: 8).  R = N + G rows in all.
 * fami_track_fill_f32: kpts [N,J,3], boxes [N,6]; fill [G,5] int: the end rows a and b (in [0, N)), the frame number f of
 *   the new row, and f_a, f_b with f_a < f < f_b -> kpts_new [G,J,3], boxes_new [G,6].  One thread per (new row, value).
 * fami_track_smooth_f32: kpts [R,J,3] (the new rows behind the first N); the members of all tracks as one list sorted by
 *   (track, frame): mrow [Mm] the row, mfr [Mm] the frame number, mtrk [Mm] the track of each, tseg [T+1] the members of
 *   track t are tseg[t] .. tseg[t+1); gauss [radius+1] fp64; radius in 1 .. 16 -> out [R,J,3]: x', y' and the confidence of
 *   every MEMBER row; other rows are not written.  out must not be kpts.  One thread per (member, joint); the window is
 *   found by walking at most `radius` members to either side (frame numbers ascend strictly within a track), so a thread
 *   makes at most 33 neighbour reads of 12 bytes.
 * fami_track_score_f32: boxes [R,6], mrow and tseg as above -> score [T], the mean of column 5 over each track's members.
 *   One thread per track, sequential over its segment.
 * No atomics, no workspace, no host read-back, every output word has one writer: bitwise reproducible.
 * Each returns -1 before any launch for a null or misaligned pointer, J outside 1 .. 32, a count < 1 (launch nothing for
 * an empty stage), R * J * 3 (fill: (N + G) * J * 3) > 2^31 - 1, T > Mm or Mm > R, fill_conf outside [0, 1], radius outside
 * 1 .. 16, a NaN threshold.  The tables are in device memory and are not checked here (evaluate.track_refine builds them):
 * every index read from one is checked against the array it addresses before use -- an end row outside [0, N) or a frame
 * number outside its gap (fill); a track outside [0, T), a segment that is no sub-range of [0, Mm] or does not hold its
 * member, a row outside [0, R) anywhere in the window (smooth); an empty or out-of-range segment, a row outside [0, R)
 * (score).  A thread whose check fails writes 1 to *flag (the caller zeroes it; every writer writes the same value) and
 * NOTHING else: nothing is read or written through such an index, and the other threads' outputs are what they would be. */
int fami_track_fill_f32(const float* kpts, const float* boxes, const int* fill, int N, int J, int G, double fill_conf,
                        float* kpts_new, float* boxes_new, int* flag, fami_stream_t stream);
int fami_track_smooth_f32(const float* kpts, const int* mrow, const int* mfr, const int* mtrk, const int* tseg,
                          const double* gauss, int R, int J, int Mm, int T, int radius, float conf_thre, float* out,
                          int* flag, fami_stream_t stream);
int fami_track_score_f32(const float* boxes, const int* mrow, const int* tseg, int R, int Mm, int T, float* score,
                         int* flag, fami_stream_t stream);

/* PoseTrack AP, the pose half of the evaluation tool the reference vendors (poseval/py/eval_helpers.py:322-367
 * removeIgnoredPoints, :453-668 assignGTmulti, :192-228 computeRPC / VOCap; evaluateAP.py:8-47 computeMetrics;
 * csrc/posetrack_ap.hip).  All pointers are DEVICE memory; fp64 arrays 8-byte, int arrays 4-byte aligned.  15 joints.
 * fami_posetrack_assign_f64: F frames; frame f owns the predicted poses pr_seg[f] .. pr_seg[f+1) (at most 256), the
 *   annotated poses gt_seg[f] .. gt_seg[f+1) (at most 64) and the ignore polygons poly_seg[f] .. poly_seg[f+1); polygon
 *   q owns the vertices vert_seg[q] .. vert_seg[q+1) of verts [NV,2] (NP and NV may be 0; vert_seg has NP + 1 entries).
 *   pr_xys [P,15,3] (x, y, score), pr_has [P] (bit j: joint j is present), gt_xy [G,15,2], gt_has [G], gt_head [G,4]
 *   (x1, y1, x2, y2).  Per frame, in fp64:
 *     1. a present point (x, y) is dropped when it lies inside any polygon of ITS frame by the even-odd rule: over the
 *        edges (i, j = i - 1 cyclically), `inside` toggles where (y_i > y) != (y_j > y) and
 *        x < (x_j - x_i) * (y - y_i) / (y_j - y_i) + x_i.  A point exactly on an edge is unspecified.
 *        pr_has_out / gt_has_out = the masks that remain (bits 0 .. 14).
 *     2. head(g) = 0.6 * sqrt((x2-x1)^2 + (y2-y1)^2); for joints both have, dist = sqrt(dx^2 + dy^2) / head(g) and
 *        match = dist <= dist_thresh (head 0: inf or NaN, no match).  pck[p,g] = #match / #joints(g), undivided when g
 *        has none.  Every p keeps only its best g (the first on ties); every g then takes the p with the largest pck
 *        among those that kept it (the first on ties; none when that is 0).
 *     label[p] = the match bits of a taken p against its g, 0 otherwise; assigned[p] = that g counted from gt_seg[f],
 *     or -1; ngt_frame[f,j] = the annotated poses of f that still have joint j.  Scores are not read here.
 *   One workgroup per frame, no atomics, no workspace: bitwise reproducible.  Returns -1 before any launch for a null or
 *   misaligned pointer (an array of extent 0 may be null), a negative extent, F < 1, P * 45, G * 30 or F * 15 >= 2^31,
 *   a NaN threshold.  The segment tables live in device memory and are not checked here
 *   (fami_pose_amd.evaluate.pack_posetrack_frames does): a frame over a cap, or with a segment that is no sub-range of
 *   its array, gets ngt_frame[f,:] = -1 and nothing else written; other frames are not affected.
 * fami_posetrack_curve_f64: lab [15,P] bytes, row j the labels (non-zero: true positive) of joint j's predictions in
 *   descending-score order, the first n_valid[j] of them valid; ngt_frame [F,15] as written above.  Per joint, with
 *   nGT = sum_f ngt_frame[f,j] and npos_k the positives among the first k + 1:
 *     precision_k = npos_k / (k+1), recall_k = npos_k / nGT, envelope_k = max(precision_k, precision_(k+1), ...),
 *     AP = sum over the k with recall_k != recall_(k-1) (recall_(-1) = 0) of (recall_k - recall_(k-1)) * envelope_k,
 *     plus (1 - recall_last) * 0 where recall_last != 1 -- VOCap with its two sentinels.
 *   out [3,16] fp64: rows ap, pre (last precision), rec (last recall), each x 100; n_valid[j] = 0 gives 0, nGT = 0 with
 *   predictions gives NaN ap and rec (0 / 0) as in the reference; column 15 = the mean over the non-NaN joints (NaN when
 *   there is none).  ngt [15] = nGT.  The AP terms are added in a fixed order (256 runs of descending k, then a binary
 *   tree): bitwise reproducible; only that order differs from numpy's sum.  Returns -1 before any launch for a null or
 *   misaligned pointer, P outside 0 .. 458752 (one label bit each in 56 KiB of LDS), F < 1. */
int fami_posetrack_assign_f64(const double* pr_xys, const int* pr_has, const double* gt_xy, const int* gt_has,
                              const double* gt_head, const int* pr_seg, const int* gt_seg, const int* poly_seg,
                              const int* vert_seg, const double* verts, int P, int G, int F, int NP, int NV,
                              double dist_thresh, int* pr_has_out, int* gt_has_out, int* label, int* assigned,
                              int* ngt_frame, fami_stream_t stream);
int fami_posetrack_curve_f64(const unsigned char* lab, const int* n_valid, const int* ngt_frame, int P, int F,
                             double* out, int* ngt, fami_stream_t stream);

/* PoseTrack MOTA, the tracking half of the same tool (poseval/py/evaluateTracking.py:13-222 computeMetrics; the `mot`
 * part of eval_helpers.assignGTmulti, :594-612, 648-658; py-motmetrics/motmetrics/mot.py:90-229 MOTAccumulator.update;
 * metrics.py:196-218 the counts; csrc/posetrack_mot.hip).  All pointers are DEVICE memory, aligned as above.
 * fami_posetrack_mot_f64: the packed arrays of fami_posetrack_assign_f64, with pr_has / gt_has the masks that entry
 *   point WROTE (pr_has_out / gt_has_out: the ignore filter runs once, MOTA and AP see the same points); pr_track [P] /
 *   gt_track [G] the track id of every pose, >= 0, the annotated ones below 256 (ids are per sequence: the caller
 *   renumbers them densely); seq_seg [S+1]: sequence s owns the kept frames seq_seg[s] .. seq_seg[s+1).  Work is per
 *   sequence and per joint j: one accumulator each, its state a map m: annotated track -> the predicted track it was
 *   last matched to (empty at the first frame).
 *   Which frames count: all of the sequence but its LAST (evaluateTracking.py:71); a sequence of one frame (the
 *   reference raises IndexError) or none contributes nothing.
 *   What a frame contributes for joint j: objects = its annotated poses that still have joint j, in order, with their
 *   track ids; hypotheses = its predicted poses that still have it.  d[o,h] = sqrt(dx^2 + dy^2) / head(o), head as
 *   above, fp64, uncontracted: the AP's expression.  A pair is valid iff d <= dist_thresh.  The reference's quirk is
 *   kept: a frame with no predicted rect or no annotated rect contributes for EVERY joint one object and one
 *   hypothesis that cannot pair (one MISS, one FP, one object), whatever the other side holds, and leaves m alone.  A
 *   rect is one that the packing kept; in a frame WITH ignore polygons, one whose mask is still non-zero.
 *   One update:
 *     1. carry forward: objects in order; if m[o] exists, is among the frame's hypotheses, is not taken in this frame
 *        and the pair is valid: MATCH with D = d, both are taken (a hypothesis that two objects remember goes to the
 *        first).
 *     2. INV = 2 * max(valid d of the frame, step 1's pairs included) + 1; a frame without a valid d skips to 3.  Taken
 *        rows and columns and invalid pairs cost INV, valid pairs d; the minimum-cost assignment of the rectangle
 *        (min(rows, columns) pairs) is solved.  Every chosen pair of cost != INV is a SWITCH if m[o] exists and differs
 *        from h, else a MATCH, D = d; then m[o] = h.  This is a minimum-COST choice, not a largest matching: the optimum
 *        may hold fewer valid pairs.  Among several optima of equal cost the choice is a function of the input alone
 *        and otherwise unspecified.
 *     3. objects left are MISSes, hypotheses left are FPs.
 *   counts [S,15,5] = num_misses, num_switches, num_false_positives, num_detections (MATCH + SWITCH), num_objects
 *   (MATCH + SWITCH + MISS); sumd [S,15] = the sum of D; status [S] = 0.  One 64-lane wavefront per (sequence, joint),
 *   shortest augmenting paths with every loop bounded by the caps, no atomics, no workspace: bitwise reproducible.
 *   Returns -1 before any launch for a null or misaligned pointer (an array of extent 0 may be null), a negative
 *   extent, F outside 1 .. (2^31 - 2) / 256, S outside 1 .. (2^31 - 2) / 75, a NaN threshold.  The tables live in device
 *   memory and are not checked here (fami_pose_amd.evaluate.pack_posetrack_frames does): a sequence whose segment is no
 *   sub-range of [0, F], or with a frame (the last excepted) over a cap (256 hypotheses, 64 objects), with a segment
 *   that is no sub-range of its array, a negative track id or an annotated one >= 256, gets status[s] = 1,
 *   counts[s,:,:] = -1, sumd[s,:] = 0 and is not processed further; other sequences are not affected.  A track id
 *   listed twice in a frame is not detected: that sequence's counts are then unspecified (nothing else is).
 * fami_posetrack_mot_final_f64: totals [15,5] and sumd_tot [15] = the sequences with status 0 added in index order;
 *   table [4,16] fp64, rows mota, motp, pre, rec (evaluateTracking.py:158-192):
 *     mota = 100 (1 - (misses + switches + fps) / objects), NaN without objects;
 *     motp = 100 (1 - sumD / detections), 0 without detections;
 *     pre = 100 detections / (fps + detections), NaN when that sum is 0;  rec = 100 detections / objects;
 *   column 15 = the mean over the non-NaN joints, in joint order (NaN when there is none). */
int fami_posetrack_mot_f64(const double* pr_xys, const int* pr_has, const double* gt_xy, const int* gt_has,
                           const double* gt_head, const int* pr_seg, const int* gt_seg, const int* poly_seg,
                           const int* pr_track, const int* gt_track, const int* seq_seg, int P, int G, int F, int S,
                           double dist_thresh, int* counts, double* sumd, int* status, fami_stream_t stream);
int fami_posetrack_mot_final_f64(const int* counts, const double* sumd, const int* status, int S, int* totals,
                                 double* sumd_tot, double* table, fami_stream_t stream);

/* COCO keypoint AP / AR: COCOeval(gt, dt, 'keypoints') of pycocotools' cocoeval.py (computeOks, evaluateImg, accumulate),
 * the number the HRNet evaluation protocol reports, for ONE category (csrc/coco_ap.hip).  pycocotools is no part of the
 * reference tree, so the definition is restated here in full and THIS TEXT IS THE CONTRACT.  Pointers are DEVICE memory
 * unless marked HOST; fp64 arrays 8-byte, int arrays 4-byte aligned.  All arithmetic is fp64 on fp64 inputs.
 * fami_coco_kpt_match_f64: M images; image m owns the annotations gt_seg[m] .. gt_seg[m+1) (at most 128) and the
 *   detections dt_seg[m] .. dt_seg[m+1) (at most 256); either may be empty.  gt_kpts [G,J,3] (x, y, v), gt_area [G],
 *   gt_bbox [G,4] (bx, by, bw, bh), gt_flags [G] (bit 0: ignore = iscrowd or num_keypoints == 0, bit 1: iscrowd);
 *   dt_kpts [D,J,3] (x, y, confidence: not read), dt_score [D] (finite), dt_area [D] (the area of the bounding box of the
 *   J (x, y) pairs, loadRes's rule; the caller computes it).  HOST: vars [J] = (2 sigma_j)^2, iou_thrs [T] (T in
 *   1 .. 32), area_rng [A,2] = (lo, hi) per range (A in 1 .. 8) -- built with numpy by the caller and never recomputed
 *   (np.linspace(.5, .95, 10)[8] is 0.8999999999999999); they travel to the kernel as launch arguments.  Per image:
 *     1. the detections are ordered by descending score, equal scores by list position (a stable sort), and the first
 *        max_dets (1 .. 64) are kept.
 *     2. for every annotation g and kept detection d, with k1 = #(vg > 0):
 *          k1 > 0:  dx = xd - xg, dy = yd - yg;
 *          k1 == 0: with x0 = bx - bw, x1 = bx + 2 bw, y0 = by - bh, y1 = by + 2 bh:
 *                   dx = max(0, x0 - xd) + max(0, xd - x1), dy = max(0, y0 - yd) + max(0, yd - y1);
 *          e_j = (dx^2 + dy^2) / vars_j / (area_g + 2^-52) / 2;
 *          OKS(d, g) = the mean of exp(-e_j) over the joints with vg > 0, over ALL joints when k1 == 0;
 *        one rounding per operation, the sum in ascending j.  (Not the OKS of fami_pose_nms_f32 / fami_pose_track_f32,
 *        which averages two areas and reads fp32.)
 *     3. per area range a: gIg(g) = ignore or area_g < lo or area_g > hi -- strict comparisons, an area of exactly lo or hi
 *        is inside, so one of exactly 32^2 or 96^2 lies in two of COCO's ranges; the annotations are ordered with the
 *        non-ignored ones first, list order otherwise (a stable argsort of gIg).
 *     4. per (a, t) and for each kept detection in score order: best = min(iou_thrs[t], 1 - 1e-10), m = none; walk the
 *        annotations in the order of 3: skip one already matched at this (a, t) unless it is a crowd annotation; STOP if
 *        m is set, m is not ignored and this one is; skip it if OKS < best; else best = OKS, m = this (an exact tie goes
 *        to the later annotation).  If m is set: the detection is matched, dIg = gIg(m), m is matched.
 *     5. an unmatched detection whose own area is < lo or > hi gets dIg = 1.
 *   out_score [M,max_dets] and out_row [M,max_dets]: the score and the row (in dt_kpts) of kept slot k of image m, 0 and
 *   -1 for a slot behind the image's last detection; out_flags [M,max_dets,A*T] bytes, index a * T + t: bit 0 matched,
 *   bit 1 dIg (0 for an empty slot); npig [M,A] = the annotations of the image with gIg = 0.  An image with neither
 *   annotations nor detections writes empty slots and npig 0; one with detections only, its detections unmatched.
 *   Deliberate differences: pycocotools decides "matched" by dtm != 0 with dtm the matched annotation's id, so an
 *   annotation with id 0 never counts there; here it is a flag.  The `scores` array of accumulate is not produced.
 *   One launch, one workgroup per image, no atomics, no workspace: bitwise reproducible.  Returns -1 before any launch for
 *   a null or misaligned pointer (an array of extent 0 may be null), G or D < 0 or G * J * 3 or D * J * 3 >= 2^31, M < 1 or
 *   M * max_dets * A * T >= 2^31, J outside 1 .. 32, T outside 1 .. 32, A outside 1 .. 8, max_dets outside 1 .. 64, a NaN
 *   in vars, iou_thrs or area_rng.  The segment tables live in device memory and are not checked here
 *   (fami_pose_amd.evaluate.pack_coco_keypoints does): an image over a cap, or with a segment that is no sub-range of
 *   its array, gets npig[m,:] = -1 and nothing else written; other images are not affected.
 * fami_coco_kpt_curve_f64: flags [A*T,N] bytes, row a * T + t the bytes of ALL kept detections of the set in descending
 *   score order (a stable sort over the images in order: the caller's); npig_img [M,A] as written above; HOST: rec_thrs
 *   [R] (R in 1 .. 256).  Per (a, t), with npig = sum_m npig_img[m,a]:
 *     npig == 0: precision[t,:,a] = recall[t,a] = -1.  Otherwise tp_k / fp_k = the number of detections among the first
 *     k + 1 with matched & !dIg / !matched & !dIg;  rc_k = tp_k / npig;  pr_k = tp_k / (fp_k + tp_k + 2^-52);
 *     recall[t,a] = rc_last (0 when N = 0);  pr_k <- max(pr_k, pr_(k+1), ...);  for each r: k = the first index with
 *     rc_k >= rec_thrs[r] (searchsorted, side left) and precision[t,r,a] = pr_k, 0 when there is none.
 *   precision [T,R,A], recall [T,A].  Every value is int -> double, one add, one add of 2^-52 and one divide, or a maximum
 *   of such values: the result equals the numpy expressions bit for bit.  N is at most 229376: two bits per detection
 *   in 56 KiB of LDS.  Returns -1 before any launch for a null or misaligned pointer (flags may be null with N = 0), N
 *   outside 0 .. 229376, M outside 1 .. (2^31 - 2) / 8, T, A or R outside their ranges, a NaN in rec_thrs.
 * The ten summary numbers (AP, AP50, AP75, AP-medium, AP-large and the five ARs) are means over the entries > -1 of
 * slices of these two arrays and are taken on the host (fami_pose_amd.evaluate.coco_keypoint_ap), as pycocotools does. */
int fami_coco_kpt_match_f64(const double* gt_kpts, const double* gt_area, const double* gt_bbox, const int* gt_flags,
                            const double* dt_kpts, const double* dt_score, const double* dt_area, const int* gt_seg,
                            const int* dt_seg, const double* vars, const double* iou_thrs, const double* area_rng, int G,
                            int D, int M, int J, int T, int A, int max_dets, double* out_score, int* out_row,
                            unsigned char* out_flags, int* npig, fami_stream_t stream);
int fami_coco_kpt_curve_f64(const unsigned char* flags, const int* npig_img, const double* rec_thrs, int N, int M, int T,
                            int A, int R, double* precision, double* recall, fami_stream_t stream);

/* ---- input pipeline on the device -------------------------------------------------------------
 * cv2.warpAffine(frame, trans, (Wd, Hd), flags=INTER_LINEAR) on the F 8-bit HWC frames of one clip (one transform
 * for key + supporting frames, datasets/zoo/posetrack/PoseTrack_Alignment.py:421-427; flip = source mirrored in x
 * first, :409-413; swap_rb = cv2.cvtColor(BGR2RGB), :299-300), then transforms.ToTensor + Normalize
 * (datasets/transforms/build.py:12-23): out[f][c][y][x] = ((crop / 255) - mean[c]) / std[c], NCHW fp32.
 * m00..m12: the INVERSE map (dst -> src) cv2 derives from `trans` (fami_pose_amd.data.invert_affine).  Coordinates and
 * interpolation follow OpenCV's generic fixed-point path bit for bit (see csrc/preproc.hip). */
int fami_warp_normalize_u8(const unsigned char* src, float* out, int F, int Hs, int Ws, long src_stride, int Hd, int Wd,
                           long out_stride, double m00, double m01, double m02, double m10, double m11, double m12,
                           int flip, int swap_rb, float mean0, float mean1, float mean2, float std0, float std1,
                           float std2, fami_stream_t stream);
/* The same crop for every frame of every clip of a BATCH in one launch: the B x (1 + supporting) cv2.warpAffine calls
 * and transforms of one minibatch (PoseTrack_Alignment.py:416-428 per sample; in evaluation many person boxes cropped
 * from the same five frames, :380-443).  Per pixel it is fami_warp_normalize_u8's arithmetic, expression for
 * expression (one shared device function): the output is bit for bit what B pairs of per-clip calls write.
 * table: DEVICE memory the caller owns, fami_warp_batch_table_bytes(B, F) bytes (-1 for B <= 0 or F <= 0), 8-byte
 *   aligned: first B fami_warp_clip_t records, then B*F source pointers `const unsigned char*`, pointer [b*F + f] = frame
 *   f of clip b ([Hs][Ws][3] 8-bit HWC, contiguous), the key frame at f = 0.  Pointers are per (clip, frame): clips may
 *   name the same frame, and the frames of a clip need not be adjacent.  All frames of a clip share the clip's Hs, Ws;
 *   clips may differ.  The table is in memory, not in the arguments, because B*F pointers outgrow the kernel-argument
 *   block at evaluation batch sizes; a workgroup reads its clip's record through a uniform index, once.
 * key [B,3,Hd,Wd], sup [B,3(F-1),Hd,Wd] fp32: frame 0 of clip b -> key[b], frame f >= 1 -> channels 3(f-1)..3f-1 of
 *   sup[b]; sup may be null when F == 1.  swap_rb, mean, std: for the whole batch.
 * Checked here (-1, no launch): null table / key, null sup with F > 1, B <= 0 (or > 65535, the grid's y extent), F <= 0,
 * Hd*Wd >= 2^31, a zero std.  The records live in device memory and are NOT checked: the caller guarantees
 * 0 < Hs, Ws < 32768 and non-null frames (fami_pose_amd.data.ClipBatcher does).  Grid: pixels x clips, one thread per
 * output pixel of all F frames; the library allocates nothing. */
typedef struct fami_warp_clip_t {
  double m[6];  /* inverse map (dst -> src) of the clip, row-major 2x3: fami_warp_normalize_u8's m00..m12 */
  int flip;     /* source mirrored in x first */
  int Hs, Ws;   /* size of every source frame of the clip */
  int reserved; /* 0 (pads the record to 64 bytes) */
} fami_warp_clip_t;
long fami_warp_batch_table_bytes(int B, int F);
int fami_warp_normalize_batch_u8(const void* table, float* key, float* sup, int B, int F, int Hd, int Wd, int swap_rb,
                                 float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                 fami_stream_t stream);
/* The batched crop with DEGRADATION of the 8-bit crop: line blur, colour, occluders.  The reference has nothing of the
 * kind (its datasets/transforms/data_augment.py is a plotting helper); the rule below is this project's and this text is
 * its contract.  Same table, grid and outputs as fami_warp_normalize_batch_u8, plus
 * degrade: DEVICE memory the caller owns, fami_degrade_table_bytes(B, F) bytes (-1 for B <= 0 or F <= 0), 8-byte
 *   aligned: B*F fami_degrade_frame_t records, record [b*F + f] for frame f of clip b (key frame at f = 0).
 * `flags` says which stages run on the frame; a stage whose flag is off is SKIPPED, not run with neutral parameters.
 * With flags == 0 in every record the output is fami_warp_normalize_batch_u8's, bit for bit.  Per output pixel (x, y),
 * 0 <= x < Wd, 0 <= y < Hd, of frame f, in this order:
 *  1. Line blur (FAMI_DEGRADE_BLUR; taps odd, 1..15; step_x, step_y integers in 1/1024 source pixel).  With
 *     (PX, PY) = (X0 + adelta, Y0 + bdelta), the un-shifted fixed-point position of the plain crop (csrc/preproc.hip),
 *     tap k = -(taps-1)/2 .. (taps-1)/2 samples at ((PX + k*step_x) >> 5, (PY + k*step_y) >> 5) exactly as the plain crop
 *     samples at (PX >> 5, PY >> 5): integer bilinear weights summing to 2^15, taps outside the image read 0, columns
 *     mirrored under the clip's `flip`; each tap gives one 8-bit value per channel, (acc + 2^14) >> 15.  The result is
 *     u_c = (2 * sum_c + taps) / (2 * taps) in integer arithmetic (the mean, rounded half up).  taps = 1 with zero steps is
 *     the plain sample.  Flag off: u_c is the plain sample.  The caller guarantees |k * step| < 2^24 for every tap.
 *  2. Colour (FAMI_DEGRADE_COLOUR; alpha, delta, sat fp32).  Every fp32 operation is rounded on its own, no contraction.
 *     Channels are the OUTPUT's (c = 0, 1, 2 are R, G, B after swap_rb):
 *       t_c = u_c * alpha + delta;   g = ((0.299f * t_0) + (0.587f * t_1)) + (0.114f * t_2);
 *       t_c = g + sat * (t_c - g);   t_c = min(max(t_c, 0), 255).
 *     The value stays a float; it is not rounded back to a byte.  Flag off: t_c = (float)u_c.
 *  3. Occluders (FAMI_DEGRADE_OCCLUDE; n_rect <= 4 rectangles in crop pixels, half-open: x0 <= x < x1, y0 <= y < y1;
 *     they may reach outside the crop or be empty).  A covered pixel takes a fill value IN PLACE of t_c:
 *       mode 0: the constant byte fill[c];
 *       mode 1: noise, lowbias32(((c * Hd + y) * Wd + x) ^ seed) >> 24 with the record's seed, everything in wrapping
 *               32-bit unsigned arithmetic; lowbias32(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b;
 *               v ^= v >> 16.
 *     Rectangles apply in order: the later one wins an overlap.  Nothing else about overlaps is defined.
 *  4. Normalisation: ((t_c / 255) - mean[c]) / std[c], as in the plain crop.
 * Checked here (-1, no launch): what fami_warp_normalize_batch_u8 checks, a null or misaligned degrade.  The records
 * live in device memory and are NOT checked: the caller guarantees odd taps in 1..15, the step bound, n_rect in 0..4 and
 * finite alpha, delta, sat (fami_pose_amd.data.ClipBatcher does; the kernel clamps taps and n_rect into range so that a
 * bad record cannot divide by zero or read past the record).  No atomics, no workspace: results are bitwise reproducible. */
#define FAMI_DEGRADE_BLUR 1
#define FAMI_DEGRADE_COLOUR 2
#define FAMI_DEGRADE_OCCLUDE 4
typedef struct fami_degrade_rect_t {
  int x0, y0, x1, y1;    /* crop pixels, half-open */
  unsigned char fill[3]; /* mode 0: the byte of output channel c */
  unsigned char mode;    /* 0 constant, 1 noise */
} fami_degrade_rect_t;
typedef struct fami_degrade_frame_t {
  unsigned int flags; /* FAMI_DEGRADE_* */
  int taps, step_x, step_y;
  float alpha, delta, sat;
  unsigned int seed;
  int n_rect;
  int reserved[3]; /* 0 (pads the record to 128 bytes) */
  fami_degrade_rect_t rect[4];
} fami_degrade_frame_t;
long fami_degrade_table_bytes(int B, int F);
int fami_warp_degrade_batch_u8(const void* table, const void* degrade, float* key, float* sup, int B, int F, int Hd,
                               int Wd, int swap_rb, float mean0, float mean1, float mean2, float std0, float std1,
                               float std2, fami_stream_t stream);


/* ======================================================================================================
 * bf16 activation storage (BASELINE config 3: bf16 compute, fp32 master weights / accumulation / losses).
 * Every entry point above that touches an activation has a `_bf16` twin with identical semantics and argument
 * order; only the activation pointers change type.  Parameters, BatchNorm statistics, workspaces, the
 * translation (tx,ty), weight gradients, DCN input-gradient accumulators and everything at the NCHW boundary
 * stay fp32.  Convolutions run on v_mfma_f32_16x16x32_bf16 with a bf16 packed weight image (KC = Cin/32).
 * ====================================================================================================== */
typedef unsigned short fami_bf16_t; /* IEEE bfloat16 bit pattern */

long fami_packed_weight_elems_bf16(int Co, int Ci, int kh, int kw, int mode);
int fami_pack_conv_weight_bf16(const float* w_oihw, fami_bf16_t* wp, int Co, int Ci, int kh, int kw, int mode,
                               fami_stream_t stream);
int fami_pack_conv_weights_batch_bf16(const float* params, fami_bf16_t* packed, const void* desc, int n,
                                      fami_stream_t stream);
/* y is bf16, or fp32 when out_f32 (heatmap-producing layers) */
int fami_conv2d_fwd_bf16(const fami_bf16_t* x, const fami_bf16_t* wp, const float* bias, void* y, int N, int H, int W,
                         int Ci, int Co, int kh, int kw, int stride, int pad, int dil, int relu, int accumulate,
                         int out_f32, fami_stream_t stream);
int fami_conv2d_dgrad_bf16(const fami_bf16_t* dy, const fami_bf16_t* wp, fami_bf16_t* dx, int N, int H, int W, int Ci,
                           int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                           fami_stream_t stream);
int fami_conv2d_fwd_xbn_bf16(const fami_bf16_t* z, const fami_bf16_t* wp, const float* bias, fami_bf16_t* y, int N, int H, int W,
                             int Ci, int Co, void* slots, const float* pivot_src, const void* xslots, long xP,
                             const float* xgamma, const float* xbeta, float* xmean, float* xinvstd,
                             float* xrunning_mean, float* xrunning_var, float xmomentum, float xeps, fami_stream_t stream);
int fami_conv2d_fwd_bnin_bf16(const fami_bf16_t* z, const fami_bf16_t* wp, const float* bias, fami_bf16_t* y, fami_bf16_t* a_out, int N, int H, int W,
                              int Ci, int Co, void* slots, const float* pivot_src, const void* xslots, long xP,
                              const float* xgamma, const float* xbeta, float* xmean, float* xinvstd,
                              float* xrunning_mean, float* xrunning_var, float xmomentum, float xeps, fami_stream_t stream);
int fami_conv2d_wgrad_defer_xbn_bf16(const fami_bf16_t* z, const fami_bf16_t* dy, float* dw, float* workspace, long ws_bytes,
                                     int N, int H, int W, int Ci, int Co, int accumulate, long* desc_out,
                                     const float* xmean, const float* xinvstd, const float* xgamma, const float* xbeta,
                                     fami_stream_t stream);
int fami_conv2d_fwd_stats_bf16(const fami_bf16_t* x, const fami_bf16_t* wp, const float* bias, fami_bf16_t* y, int N, int H, int W,
                               int Ci, int Co, int kh, int kw, int stride, int pad, int dil, void* slots,
                               const float* pivot_src, fami_stream_t stream);
int fami_conv2d_dgrad_bnstats_bf16(const fami_bf16_t* dy, const fami_bf16_t* wp, fami_bf16_t* dx, int N, int H, int W, int Ci,
                                   int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                                   const fami_bf16_t* z, const fami_bf16_t* yrelu, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, int relu, void* slots, fami_stream_t stream);
int fami_conv2d_bwd_pair_bf16(const fami_bf16_t* x, const fami_bf16_t* dy, const fami_bf16_t* wpd, fami_bf16_t* dx, float* dw, float* workspace,
                              long ws_bytes, int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad,
                              int dil, int acc_dx, int acc_dw, long* desc_out, const fami_bf16_t* z, const fami_bf16_t* yrelu,
                              const float* mean, const float* invstd, const float* gamma, const float* beta, int relu,
                              void* slots, fami_stream_t stream);
int fami_bn_apply_slots_bf16(const fami_bf16_t* x, const fami_bf16_t* residual, fami_bf16_t* y, const float* gamma,
                             const float* beta, float* mean, float* invstd, float* running_mean, float* running_var,
                             long P, int C, int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd_apply_slots_bf16(const fami_bf16_t* dz, const fami_bf16_t* x, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, fami_bf16_t* dx, float* dgamma, float* dbeta,
                                 fami_bf16_t* dres, long P, int C, int acc_dx, int acc_param, int acc_dres, void* slots,
                                 fami_stream_t stream);
int fami_conv2d_wgrad_defer_bf16(const fami_bf16_t* x, const fami_bf16_t* dy, float* dw, float* workspace, long ws_bytes,
                                 int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                                 int accumulate, long* desc_out, fami_stream_t stream);
int fami_conv2d_wgrad_bf16(const fami_bf16_t* x, const fami_bf16_t* dy, float* dw, float* workspace, long ws_bytes,
                           int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                           int accumulate, fami_stream_t stream);

int fami_bn_stats_bf16(const fami_bf16_t* x, long P, int C, float* mean, float* invstd, float* running_mean,
                       float* running_var, float momentum, float eps, float* ws, fami_stream_t stream);
int fami_bn_train_fwd_bf16(const fami_bf16_t* x, const fami_bf16_t* residual, fami_bf16_t* y, const float* gamma,
                           const float* beta, float* mean, float* invstd, float* running_mean, float* running_var,
                           long P, int C, int relu, float momentum, float eps, float* ws, fami_stream_t stream);
int fami_bn_apply_bf16(const fami_bf16_t* x, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, const fami_bf16_t* residual, fami_bf16_t* y, long P, int C, int relu,
                       fami_stream_t stream);
int fami_bn_train_fwd2_bf16(const fami_bf16_t* x, const fami_bf16_t* residual, fami_bf16_t* y, const float* gamma, const float* beta,
                           float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,
                           int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd2_bf16(const fami_bf16_t* dy, const fami_bf16_t* x, const fami_bf16_t* y, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, fami_bf16_t* dx, float* dgamma, float* dbeta, fami_bf16_t* dres, long P,
                     int C, int relu, int acc_dx, int acc_param, int acc_dres, void* slots, fami_stream_t stream);
int fami_bn_bwd_bf16(const fami_bf16_t* dy, const fami_bf16_t* x, const fami_bf16_t* y, const float* mean,
                     const float* invstd, const float* gamma, fami_bf16_t* dx, float* dgamma, float* dbeta,
                     fami_bf16_t* dres, long P, int C, int relu, int acc_dx, int acc_param, int acc_dres, float* ws,
                     fami_stream_t stream);
int fami_bn_eval_bwd_bf16(const fami_bf16_t* dy, const fami_bf16_t* x, const fami_bf16_t* y, const float* mean,
                     const float* invstd, const float* gamma, fami_bf16_t* dx, float* dgamma, float* dbeta,
                     fami_bf16_t* dres, long P, int C, int relu, int acc_dx, int acc_param, int acc_dres, float* ws,
                     fami_stream_t stream);
int fami_channel_sum_bf16(const fami_bf16_t* x, long P, int C, float* out, int accumulate, float* ws,
                          fami_stream_t stream);

int fami_nchw_to_nhwc_bf16(const float* src, fami_bf16_t* dst, int N, int C, int H, int W, fami_stream_t stream);
int fami_nhwc_to_nchw_bf16(const fami_bf16_t* src, float* dst, int N, int C, int H, int W, int accumulate,
                           fami_stream_t stream);
int fami_pack_frames_bf16(const float* kf_nchw, const float* sup_nchw, fami_bf16_t* frames_nhwc, int B, int S, int H,
                          int W, fami_stream_t stream);
int fami_copy_channels_bf16(const fami_bf16_t* src, fami_bf16_t* dst, long P, int Cs, int src_off, int Cd,
                            int dst_off, int Cc, int accumulate, fami_stream_t stream);
/* torch.cat on channels of n <= 4 tensors in one launch (c[k] % 4 == 0) and its backward: the k-th channel slice of src (=|+=) into
 * dst[k] (null: skipped).  src / dst / c / accumulate are HOST arrays of length n. */
int fami_concat_channels_bf16(const fami_bf16_t* const* src, const int* c, int n, fami_bf16_t* dst, long P, fami_stream_t stream);
int fami_split_channels_bf16(const fami_bf16_t* src, fami_bf16_t* const* dst, const int* c, const int* accumulate, int n, long P,
                             fami_stream_t stream);
int fami_axpby_bf16(const fami_bf16_t* a, const fami_bf16_t* b, fami_bf16_t* out, long n, float alpha, float beta,
                    fami_stream_t stream);
int fami_widen_bf16(const fami_bf16_t* src, float* dst, long n, fami_stream_t stream);
int fami_cast_add_bf16(const float* src, fami_bf16_t* dst, long n, int accumulate, fami_stream_t stream);
int fami_fill_bf16(fami_bf16_t* out, long n, float v, fami_stream_t stream);
int fami_fuse_sum_bf16(int nterms, const fami_bf16_t* const* x, const float* const* mean, const float* const* invstd,
                       const float* const* gamma, const float* const* beta, const int* shift, fami_bf16_t* y, int N,
                       int H, int W, int C, int relu, fami_stream_t stream);
int fami_relu_bwd_bf16(const fami_bf16_t* dy, const fami_bf16_t* y, fami_bf16_t* dx, long n, int accumulate,
                       fami_stream_t stream);
int fami_pool_relu_bwd_bf16(const fami_bf16_t* dy, const fami_bf16_t* y, fami_bf16_t* out, int N, int Hl, int Wl,
                            int C, int shift, int relu, fami_stream_t stream);

int fami_shift_bilinear_fwd_bf16(const fami_bf16_t* src, const float* t, fami_bf16_t* out, int B, int H, int W, int C,
                                 fami_stream_t stream);
int fami_shift_bilinear_bwd_bf16(const fami_bf16_t* gout, const fami_bf16_t* src, const float* t, fami_bf16_t* gsrc,
                                 float* gt, int B, int H, int W, int C, int acc_src, int acc_t, float* ws,
                                 fami_stream_t stream);
int fami_dcn_fwd_bf16(const fami_bf16_t* x, const fami_bf16_t* off, const fami_bf16_t* msk, const float* wp,
                      const float* bias, fami_bf16_t* y, int B, int H, int W, int C, int Co, int G, int kh, int kw,
                      int stride, int pad, int dil, fami_stream_t stream);
int fami_dcn_bwd_bf16(const fami_bf16_t* x, const fami_bf16_t* off, const fami_bf16_t* msk, const fami_bf16_t* dy,
                      const float* wpb, fami_bf16_t* col, float* gx, fami_bf16_t* goff, fami_bf16_t* gmsk, int B,
                      int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, int acc_off,
                      fami_stream_t stream);
int fami_dcn_bwd_det_bf16(const fami_bf16_t* x, const fami_bf16_t* off, const fami_bf16_t* msk, const fami_bf16_t* dy, const float* wpb, fami_bf16_t* col,
                         fami_bf16_t* gx, fami_bf16_t* goff, fami_bf16_t* gmsk, int B, int H, int W, int C, int Co, int G, int kh, int kw,
                         int stride, int pad, int dil, int acc_off, int acc_x, void* ws, fami_stream_t stream);
int fami_dcn_fwd_om_bf16(const fami_bf16_t* x, const fami_bf16_t* om, const float* wp, const float* bias, fami_bf16_t* y, int B, int H, int W,
                       int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, fami_stream_t stream);
int fami_dcn_bwd_om_bf16(const fami_bf16_t* x, const fami_bf16_t* om, const fami_bf16_t* dy, const float* wpb, fami_bf16_t* col, float* gx, fami_bf16_t* gom,
                       int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, int acc_om,
                       fami_stream_t stream);
int fami_dcn_bwd_det_om_bf16(const fami_bf16_t* x, const fami_bf16_t* om, const fami_bf16_t* dy, const float* wpb, fami_bf16_t* col, fami_bf16_t* gx,
                           fami_bf16_t* gom, int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad,
                           int dil, int acc_om, int acc_x, void* ws, fami_stream_t stream);


/* ======================================================================================================
 * fp16 activation storage (BASELINE config 5: "fp16 MFMA convs + fp32 loss accumulation").  Identical in every
 * respect to the bf16 family above -- same argument order, same fp32 accumulation / BatchNorm statistics / master
 * weights / losses -- with IEEE binary16 storage and v_mfma_f32_16x16x32_f16.  The packed weight image has the
 * bf16 geometry.  (posetimation/backbones/hrnet.py:569-629 driven by STAGE*.NUM_CHANNELS = 64/128/256/512.)
 * ====================================================================================================== */
typedef unsigned short fami_f16_t; /* IEEE binary16 bit pattern */

long fami_packed_weight_elems_f16(int Co, int Ci, int kh, int kw, int mode);
int fami_pack_conv_weight_f16(const float* w_oihw, fami_f16_t* wp, int Co, int Ci, int kh, int kw, int mode,
                               fami_stream_t stream);
int fami_pack_conv_weights_batch_f16(const float* params, fami_f16_t* packed, const void* desc, int n,
                                      fami_stream_t stream);
/* y is fp16, or fp32 when out_f32 (heatmap-producing layers) */
int fami_conv2d_fwd_f16(const fami_f16_t* x, const fami_f16_t* wp, const float* bias, void* y, int N, int H, int W,
                         int Ci, int Co, int kh, int kw, int stride, int pad, int dil, int relu, int accumulate,
                         int out_f32, fami_stream_t stream);
int fami_conv2d_dgrad_f16(const fami_f16_t* dy, const fami_f16_t* wp, fami_f16_t* dx, int N, int H, int W, int Ci,
                           int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                           fami_stream_t stream);
int fami_conv2d_fwd_xbn_f16(const fami_f16_t* z, const fami_f16_t* wp, const float* bias, fami_f16_t* y, int N, int H, int W,
                             int Ci, int Co, void* slots, const float* pivot_src, const void* xslots, long xP,
                             const float* xgamma, const float* xbeta, float* xmean, float* xinvstd,
                             float* xrunning_mean, float* xrunning_var, float xmomentum, float xeps, fami_stream_t stream);
int fami_conv2d_fwd_bnin_f16(const fami_f16_t* z, const fami_f16_t* wp, const float* bias, fami_f16_t* y, fami_f16_t* a_out, int N, int H, int W,
                              int Ci, int Co, void* slots, const float* pivot_src, const void* xslots, long xP,
                              const float* xgamma, const float* xbeta, float* xmean, float* xinvstd,
                              float* xrunning_mean, float* xrunning_var, float xmomentum, float xeps, fami_stream_t stream);
int fami_conv2d_wgrad_defer_xbn_f16(const fami_f16_t* z, const fami_f16_t* dy, float* dw, float* workspace, long ws_bytes,
                                     int N, int H, int W, int Ci, int Co, int accumulate, long* desc_out,
                                     const float* xmean, const float* xinvstd, const float* xgamma, const float* xbeta,
                                     fami_stream_t stream);
int fami_conv2d_fwd_stats_f16(const fami_f16_t* x, const fami_f16_t* wp, const float* bias, fami_f16_t* y, int N, int H, int W,
                               int Ci, int Co, int kh, int kw, int stride, int pad, int dil, void* slots,
                               const float* pivot_src, fami_stream_t stream);
int fami_conv2d_dgrad_bnstats_f16(const fami_f16_t* dy, const fami_f16_t* wp, fami_f16_t* dx, int N, int H, int W, int Ci,
                                   int Co, int kh, int kw, int stride, int pad, int dil, int accumulate,
                                   const fami_f16_t* z, const fami_f16_t* yrelu, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, int relu, void* slots, fami_stream_t stream);
int fami_conv2d_bwd_pair_f16(const fami_f16_t* x, const fami_f16_t* dy, const fami_f16_t* wpd, fami_f16_t* dx, float* dw, float* workspace,
                              long ws_bytes, int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad,
                              int dil, int acc_dx, int acc_dw, long* desc_out, const fami_f16_t* z, const fami_f16_t* yrelu,
                              const float* mean, const float* invstd, const float* gamma, const float* beta, int relu,
                              void* slots, fami_stream_t stream);
int fami_bn_apply_slots_f16(const fami_f16_t* x, const fami_f16_t* residual, fami_f16_t* y, const float* gamma,
                             const float* beta, float* mean, float* invstd, float* running_mean, float* running_var,
                             long P, int C, int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd_apply_slots_f16(const fami_f16_t* dz, const fami_f16_t* x, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, fami_f16_t* dx, float* dgamma, float* dbeta,
                                 fami_f16_t* dres, long P, int C, int acc_dx, int acc_param, int acc_dres, void* slots,
                                 fami_stream_t stream);
int fami_conv2d_wgrad_defer_f16(const fami_f16_t* x, const fami_f16_t* dy, float* dw, float* workspace, long ws_bytes,
                                 int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                                 int accumulate, long* desc_out, fami_stream_t stream);
int fami_conv2d_wgrad_f16(const fami_f16_t* x, const fami_f16_t* dy, float* dw, float* workspace, long ws_bytes,
                           int N, int H, int W, int Ci, int Co, int kh, int kw, int stride, int pad, int dil,
                           int accumulate, fami_stream_t stream);

int fami_bn_stats_f16(const fami_f16_t* x, long P, int C, float* mean, float* invstd, float* running_mean,
                       float* running_var, float momentum, float eps, float* ws, fami_stream_t stream);
int fami_bn_train_fwd_f16(const fami_f16_t* x, const fami_f16_t* residual, fami_f16_t* y, const float* gamma,
                           const float* beta, float* mean, float* invstd, float* running_mean, float* running_var,
                           long P, int C, int relu, float momentum, float eps, float* ws, fami_stream_t stream);
int fami_bn_apply_f16(const fami_f16_t* x, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, const fami_f16_t* residual, fami_f16_t* y, long P, int C, int relu,
                       fami_stream_t stream);
int fami_bn_train_fwd2_f16(const fami_f16_t* x, const fami_f16_t* residual, fami_f16_t* y, const float* gamma, const float* beta,
                           float* mean, float* invstd, float* running_mean, float* running_var, long P, int C,
                           int relu, float momentum, float eps, void* slots, fami_stream_t stream);
int fami_bn_bwd2_f16(const fami_f16_t* dy, const fami_f16_t* x, const fami_f16_t* y, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, fami_f16_t* dx, float* dgamma, float* dbeta, fami_f16_t* dres, long P,
                     int C, int relu, int acc_dx, int acc_param, int acc_dres, void* slots, fami_stream_t stream);
int fami_bn_bwd_f16(const fami_f16_t* dy, const fami_f16_t* x, const fami_f16_t* y, const float* mean,
                     const float* invstd, const float* gamma, fami_f16_t* dx, float* dgamma, float* dbeta,
                     fami_f16_t* dres, long P, int C, int relu, int acc_dx, int acc_param, int acc_dres, float* ws,
                     fami_stream_t stream);
int fami_bn_eval_bwd_f16(const fami_f16_t* dy, const fami_f16_t* x, const fami_f16_t* y, const float* mean,
                     const float* invstd, const float* gamma, fami_f16_t* dx, float* dgamma, float* dbeta,
                     fami_f16_t* dres, long P, int C, int relu, int acc_dx, int acc_param, int acc_dres, float* ws,
                     fami_stream_t stream);
int fami_channel_sum_f16(const fami_f16_t* x, long P, int C, float* out, int accumulate, float* ws,
                          fami_stream_t stream);

int fami_nchw_to_nhwc_f16(const float* src, fami_f16_t* dst, int N, int C, int H, int W, fami_stream_t stream);
int fami_nhwc_to_nchw_f16(const fami_f16_t* src, float* dst, int N, int C, int H, int W, int accumulate,
                           fami_stream_t stream);
int fami_pack_frames_f16(const float* kf_nchw, const float* sup_nchw, fami_f16_t* frames_nhwc, int B, int S, int H,
                          int W, fami_stream_t stream);
int fami_copy_channels_f16(const fami_f16_t* src, fami_f16_t* dst, long P, int Cs, int src_off, int Cd,
                            int dst_off, int Cc, int accumulate, fami_stream_t stream);
/* torch.cat on channels of n <= 4 tensors in one launch (c[k] % 4 == 0) and its backward: the k-th channel slice of src (=|+=) into
 * dst[k] (null: skipped).  src / dst / c / accumulate are HOST arrays of length n. */
int fami_concat_channels_f16(const fami_f16_t* const* src, const int* c, int n, fami_f16_t* dst, long P, fami_stream_t stream);
int fami_split_channels_f16(const fami_f16_t* src, fami_f16_t* const* dst, const int* c, const int* accumulate, int n, long P,
                             fami_stream_t stream);
int fami_axpby_f16(const fami_f16_t* a, const fami_f16_t* b, fami_f16_t* out, long n, float alpha, float beta,
                    fami_stream_t stream);
int fami_widen_f16(const fami_f16_t* src, float* dst, long n, fami_stream_t stream);
int fami_cast_add_f16(const float* src, fami_f16_t* dst, long n, int accumulate, fami_stream_t stream);
int fami_fill_f16(fami_f16_t* out, long n, float v, fami_stream_t stream);
int fami_fuse_sum_f16(int nterms, const fami_f16_t* const* x, const float* const* mean, const float* const* invstd,
                       const float* const* gamma, const float* const* beta, const int* shift, fami_f16_t* y, int N,
                       int H, int W, int C, int relu, fami_stream_t stream);
int fami_relu_bwd_f16(const fami_f16_t* dy, const fami_f16_t* y, fami_f16_t* dx, long n, int accumulate,
                       fami_stream_t stream);
int fami_pool_relu_bwd_f16(const fami_f16_t* dy, const fami_f16_t* y, fami_f16_t* out, int N, int Hl, int Wl,
                            int C, int shift, int relu, fami_stream_t stream);

int fami_shift_bilinear_fwd_f16(const fami_f16_t* src, const float* t, fami_f16_t* out, int B, int H, int W, int C,
                                 fami_stream_t stream);
int fami_shift_bilinear_bwd_f16(const fami_f16_t* gout, const fami_f16_t* src, const float* t, fami_f16_t* gsrc,
                                 float* gt, int B, int H, int W, int C, int acc_src, int acc_t, float* ws,
                                 fami_stream_t stream);
int fami_dcn_fwd_f16(const fami_f16_t* x, const fami_f16_t* off, const fami_f16_t* msk, const float* wp,
                      const float* bias, fami_f16_t* y, int B, int H, int W, int C, int Co, int G, int kh, int kw,
                      int stride, int pad, int dil, fami_stream_t stream);
int fami_dcn_bwd_f16(const fami_f16_t* x, const fami_f16_t* off, const fami_f16_t* msk, const fami_f16_t* dy,
                      const float* wpb, fami_f16_t* col, float* gx, fami_f16_t* goff, fami_f16_t* gmsk, int B,
                      int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, int acc_off,
                      fami_stream_t stream);
int fami_dcn_bwd_det_f16(const fami_f16_t* x, const fami_f16_t* off, const fami_f16_t* msk, const fami_f16_t* dy, const float* wpb, fami_f16_t* col,
                         fami_f16_t* gx, fami_f16_t* goff, fami_f16_t* gmsk, int B, int H, int W, int C, int Co, int G, int kh, int kw,
                         int stride, int pad, int dil, int acc_off, int acc_x, void* ws, fami_stream_t stream);
int fami_dcn_fwd_om_f16(const fami_f16_t* x, const fami_f16_t* om, const float* wp, const float* bias, fami_f16_t* y, int B, int H, int W,
                       int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, fami_stream_t stream);
int fami_dcn_bwd_om_f16(const fami_f16_t* x, const fami_f16_t* om, const fami_f16_t* dy, const float* wpb, fami_f16_t* col, float* gx, fami_f16_t* gom,
                       int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad, int dil, int acc_om,
                       fami_stream_t stream);
int fami_dcn_bwd_det_om_f16(const fami_f16_t* x, const fami_f16_t* om, const fami_f16_t* dy, const float* wpb, fami_f16_t* col, fami_f16_t* gx,
                           fami_f16_t* gom, int B, int H, int W, int C, int Co, int G, int kh, int kw, int stride, int pad,
                           int dil, int acc_om, int acc_x, void* ws, fami_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FAMI_H */
