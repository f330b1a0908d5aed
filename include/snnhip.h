/*
 * snnhip.h -- C ABI of libsnnhip.so: the MI355X (gfx950) implementation of BindsNET's
 * per-timestep Network.run() hot path.
 *
 * BindsNET has no FFI / operator-plugin interface of its own (it is pure Python on PyTorch),
 * so the entry points below are what a binding of that path needs: one per reference function
 * of SURVEY.md section 8(a), plus the multi-step driver snn_net_run.  Each declaration cites the
 * reference function it replaces (paths relative to the BindsNET repository root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Every pointer is a DEVICE pointer unless the
 *     parameter name starts with `h_`.  The caller owns every buffer, scratch included;
 *     the library allocates no device memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All calls are
 *     asynchronous and stream-ordered; none synchronises the device.
 *   - return value: 0 = SNN_OK, negative = error (snn_error_string()).  No C++ exception ever
 *     crosses the boundary.
 *   - arithmetic: IEEE binary32, round-to-nearest-even, no FMA contraction; every reduction
 *     follows the order the reference executes on CPU (ATen cascade sum: SURVEY.md Appendix A;
 *     serial order, see DESIGN.md "Summation order").  Spikes are uint8 (0/1), row-major
 *     [B, n]; weights are float32 row-major [Nin, N] (source-major, like BindsNET's `w`).
 */
#ifndef SNNHIP_H
#define SNNHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNN_ABI_VERSION 8

typedef void *snn_stream_t;

enum {
    SNN_OK = 0,
    SNN_ERR_INVALID = -1,      /* bad argument (null pointer, non-positive size, ...) */
    SNN_ERR_UNSUPPORTED = -2,  /* size outside what the kernels were built for */
    SNN_ERR_LAUNCH = -3,       /* hip launch / runtime error (see snn_last_hip_error) */
    SNN_ERR_NOISE = -4,        /* one_spike noise stream exhausted (device status word) */
    SNN_ERR_NO_DEVICE = -5,
    SNN_ERR_TIMEOUT = -6,      /* an in-kernel workgroup hand-off gave up waiting (device status word) */
    SNN_ERR_RETRY = -7         /* the lean form of a plan met a step it does not handle (device status word): no state
                                  was touched; run the same input again with snn_run_desc.plan = 3 */
};

int snn_abi_version(void);
const char *snn_error_string(int code);
/* hipGetErrorString() of the last failing HIP call made by this library on this thread. */
const char *snn_last_hip_error(void);
/* Number of visible HIP devices, or SNN_ERR_NO_DEVICE. */
int snn_device_count(void);

/* ---- a5: MulticompartmentConnection.compute + Weight.compute -------------------------------
 * bindsnet/network/topology.py:437-479, bindsnet/network/topology_features.py:633-645
 * out[b,j] (+)= sum_i W[i,j] * s[b,i] in ATen sum(dim=1) order (cascade over i for columns
 * j < 32*floor(N/32), 4-lane row_sum for the rest).  accumulate=0: out = 0 + r;
 * accumulate=1: out = out + r (network.py:240-248, connection insertion order).
 * Limits: Nin <= 2^19.                                                                     */
int snn_prop_cascade_f32(const float *W, const uint8_t *s, float *out,
                         int B, int Nin, int N, int accumulate, snn_stream_t stream);

/* ---- f8: MulticompartmentConnection.compute with a feature pipeline ------------------------------
 * bindsnet/network/topology.py:437-479 + bindsnet/network/topology_features.py (Probability :425-429, Mask :507-508, Weight
 * :633-645, Bias :711-712, Intensity :755-756).  The pipeline is a program of up to SNN_MCC_MAX_PIPE ops applied, in order, to
 * float(s[b,i]) per synapse (i, j):
 *   SNN_MCC_OP_MUL_DRAW  t = t * bit(i,j)    a Probability: bit from the [S, ceil(N/32)] mask snn_mcc_bernoulli wrote into `bits`
 *   SNN_MCC_OP_MUL_MASK  t = t * (val != 0)  a Mask: val is the bool / u8 [S, N] tensor
 *   SNN_MCC_OP_MUL_F32   t = t * val         a Weight or an Intensity, f32 [S, N]
 *   SNN_MCC_OP_ADD_F32   t = t + val         a Bias, f32 [S, N]
 * `scalar` != 0: val has one element, used for every synapse.  Every op is one rounded f32 multiply or add (no select).
 * (ABI 8, additive)                                                                                                       */
#define SNN_MCC_MAX_PIPE 8
enum { SNN_MCC_OP_MUL_DRAW = 1, SNN_MCC_OP_MUL_MASK = 2, SNN_MCC_OP_MUL_F32 = 3, SNN_MCC_OP_ADD_F32 = 4 };
typedef struct { int kind; int scalar; const void *val; const uint32_t *bits; } snn_mcc_op;
/* out[b,j] (+)= sum_i term(b,i,j) in ATen sum(dim=1) order, accumulate as in snn_prop_cascade_f32.  h_ops is a HOST array.
 * Without an ADD op the rows of silent sources are skipped (their terms are +-0: the values must be finite); with one the
 * walk is dense.  Limits: Nin <= 2^19.                                                                                   */
int snn_prop_mcc_pipe_f32(const snn_mcc_op *h_ops, int n_ops, const uint8_t *s, float *out, int B, int Nin, int N,
                          int accumulate, snn_stream_t stream);

/* ---- a6: Connection.compute ---------------------------------------------------------------
 * bindsnet/network/topology.py:332-346.  out[b,j] (+)= sum_i s[b,i]*W[i,j] (+ bias[j]),
 * canonical ascending-i sequential f32 (the reference's MKL order is not reproducible,
 * SURVEY.md finding 5).  bias may be NULL.                                                  */
int snn_prop_dense_f32(const float *W, const float *bias, const uint8_t *s, float *out,
                       int B, int Nin, int N, int accumulate, snn_stream_t stream);

/* ---- f9: SparseConnection.compute -----------------------------------------------------------
 * bindsnet/network/topology.py:2009-2017 + :332-346: `s.view(B, -1).float() @ w (+ b)` with `w` a sparse COO tensor.
 * Order contract: out[b,j] (+)= (...((0 + w[i1,j]) + w[i2,j]) + ...) + bias[j] over the STORED entries of column j whose
 * source i spiked, i ascending, one rounded f32 add per term, bias (nullable) last; accumulate as in snn_prop_cascade_f32.
 * This IS the reference's own order (probed at 1 and 8 threads, DESIGN.md "Summation order"), so unlike snn_prop_dense_f32
 * the result is bit-identical to the reference for float weights too.  A spike byte enters as float(s) * w, one rounded
 * multiply before the add; silent sources are skipped.  The contract is pinned against the reference for spike bytes 0/1
 * and finite weights.  Stored entries are those `to_sparse()` keeps (exact zeros and -0 are absent) after coalescing.
 * Compiled form (a column-tiled CSR, built by the caller): the N columns are cut into tiles of SNN_SPARSE_TJ; entries are
 * laid out tile by tile, inside a tile by (source, target) ascending.  ptr int32 [ceil(N/SNN_SPARSE_TJ) * Nin + 1]: the
 * entries of (tile t, source i) are [ptr[t*Nin + i], ptr[t*Nin + i + 1]); col uint8 [nnz]: the column inside the tile;
 * val f32 [nnz].  col / val may be NULL when nnz == 0.  Every segment bound is clamped into [0, nnz] on the device.
 * No float atomics.  Limits (int32 indices): nnz < 2^31, Nin <= 2^24, ceil(N/SNN_SPARSE_TJ) * Nin < 2^31 - 1, B <= 65535;
 * beyond them SNN_ERR_UNSUPPORTED.  (ABI 8, additive)                                                                      */
#define SNN_SPARSE_TJ 256
int snn_prop_sparse_f32(const int *ptr, const uint8_t *col, const float *val, int nnz, const float *bias, const uint8_t *s,
                        float *out, int B, int Nin, int N, int accumulate, snn_stream_t stream);

/* ---- f11: MaxPool1d / 2d / 3dConnection.compute -------------------------------------------------
 * bindsnet/network/topology.py:1028-1301.  fr f32 [B, C, in[0], in[1], in[2]] is the connection's `firing_rates` (updated in
 * place), s the source's spike bytes of the same shape, out f32 [B, C, out[0], out[1], out[2]] with
 * out[a] = (in[a] + 2 pad[a] - dil[a] (k[a] - 1) - 1) / stride[a] + 1.  Per call:
 *   fr = fr - decay * fr (one rounded multiply, one rounded subtract); fr = fr + float(s);
 *   idx = the index F.max_poolNd(fr, ..., return_indices=True) returns: the window's in-bounds taps in row-major order, the
 *         first in-bounds tap to begin with, replaced iff val > max || isnan(val) (first maximum, last NaN);
 *   out (+)= float(s[idx]).
 * in / k / stride / pad / dil are HOST arrays of three ints; a 1-D or 2-D pooling pads the leading dimensions with size 1,
 * kernel 1, stride 1, padding 0, dilation 1.  A plane (in[0] * in[1] * in[2]) of at most SNN_POOL_STAGE elements is updated
 * and pooled in LDS by ONE launch; a larger one takes two launches (rates, then pooling from global memory); both give the
 * same bits.  2 * pad[a] > dil[a] (k[a] - 1) + 1 (torch refuses it) or an empty output is SNN_ERR_INVALID; planes, plane sizes
 * or B * C beyond 2^30, or more than 2^40 elements, SNN_ERR_UNSUPPORTED.  (ABI 8, additive)                              */
#define SNN_POOL_STAGE 8192
int snn_prop_pool_f32(float *fr, const uint8_t *s, float *out, int B, int C, const int *in, const int *k, const int *stride,
                      const int *pad, const int *dil, float decay, int accumulate, snn_stream_t stream);

/* ---- f11: MeanFieldConnection.compute -------------------------------------------------------------
 * bindsnet/network/topology.py:1972-1981: `s.float().mean() * w`, the mean over the WHOLE [B, n_src] tensor.  The spikes are
 * counted as integers; mean = f32(count) / f32(B * n_src), one correctly rounded divide (exact operands: B * n_src <= 2^24,
 * else SNN_ERR_UNSUPPORTED; pinned for spike bytes 0/1); out[o] (+)= mean * w[o % w_numel] for o < B * n_tgt: one rounded
 * multiply, one rounded add.  w_numel is 1 (a 0-dim `w`) or the element count of a `w` whose shape is a tail of
 * [B, n_tgt...]; it must divide B * n_tgt.  accumulate: 0 -- out = 0 + mean * w, the first term of a zeroed sum as in
 * snn_prop_cascade_f32; 1 -- out = out + mean * w; SNN_MEANFIELD_STORE -- out = mean * w itself (compute()'s own value: a
 * zero keeps its sign).  One launch, no host synchronisation.  (ABI 8, additive)                                          */
#define SNN_MEANFIELD_STORE 2
int snn_prop_meanfield_f32(const float *w, int w_numel, const uint8_t *s, float *out, int B, int n_src, int n_tgt,
                           int accumulate, snn_stream_t stream);

/* The same product on the f32 matrix cores (v_mfma_f32_16x16x4_f32): ONE k-ordered accumulator chain per output
 * tile, bit-identical to snn_prop_dense_f32 when every spike byte is 0 or 1 (products are then exact and gfx950's
 * f32 MFMA is a k-ordered fmaf chain).  Cost is Nin / 4 dependent MFMAs per tile regardless of sparsity; kept as an
 * operator for dense inputs and as the measured alternative to the event-driven kernel (profiles/).   */
int snn_prop_dense_mfma_f32(const float *W, const float *bias, const uint8_t *s, float *out,
                            int B, int Nin, int N, int accumulate, snn_stream_t stream);

/* snn_prop_dense_f32 with its body chosen ON THE DEVICE, per tile of 16 samples and per call: the matrix-core chain above for
 * a tile whose spikes are dense, the event-driven walk for the others.  `out` has snn_prop_dense_f32's bits whichever body
 * runs.  Two launches, always the same two, no host read-back: the matrix kernel first -- every workgroup of a tile counts the
 * non-zero spike bytes of the tile's valid rows and notes any byte above 1 (csrc/snn_dense_auto.hpp: the census), all of them
 * reach the same decision, a tile that decides "event" returns there, the first column group of a tile writes flags[tile]
 * (1 = the matrix body has stored this tile) and adds 1 to counters[0] (matrix) or counters[1] (event) --, then the
 * event-driven kernel, whose workgroups of a flagged tile return at once.
 * A tile takes the matrix body only if (a) every spike byte of its valid rows is 0 or 1 -- another byte makes k_prop's
 * multiply-then-add two roundings where the MFMA has one -- and (b) the cost rule of csrc/snn_dense_auto.hpp says the walk of
 * the tile's longest event list costs more than Nin / 16 rounds of the chain.  (b) costs time when it is wrong, never bits.
 * flags: int32 [ceil(B / 16)], written on every call (no memset needed); counters: nullable int32 [2], only ever added to.
 * Limit: a non-finite weight in a row that did not spike gives NaN in the matrix body (0 * inf, as a matmul does) and is
 * not seen by the event-driven body.  Limits of snn_prop_dense_f32: Nin < 2^24, B <= 65535.  (ABI 8, additive)              */
int snn_prop_dense_auto_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Nin, int N,
                            int accumulate, int *flags, int *counters, snn_stream_t stream);
/* Which body snn_prop_dense_auto_f32 takes, for tests and measurements (process-wide, like snn_set_plan_mode): 0 = the
 * rule above, 1 = always the event-driven body, 2 = the matrix body wherever it is exact (a tile with a byte above 1 still
 * takes the event-driven body).  Another value is taken as 0.                                                              */
void snn_set_dense_prop_mode(int mode);

/* ---- a7: Conv2dConnection.compute ---------------------------------------------------------
 * bindsnet/network/topology.py:799-815 (F.conv2d).  s [B,Cin,H,W] u8, W [Cout,Cin,KH,KW],
 * out [B,Cout,OH,OW].  Stated order, any Cin: every output element is ONE bias-free sequential f32 sum over (kh,kw,cin) --
 * taps row-major, input channels innermost, out-of-image taps skipped, one rounding per multiply and per add --, then + bias;
 * out (+)= that.  The device equals this order (oracle: orc_prop_conv2d) bit for bit for any weights.  Against the reference:
 * Cin <= 16 -- it is what the reference's oneDNN kernel does (bit-exact against reference fixtures for Cin = 1, 3, 8, 16);
 * Cin > 16 -- oneDNN takes blocked kernels whose order depends on the host's ISA: equal bit for bit whenever every partial sum
 * is exactly representable (fixtures with weights on a 1/64 grid), else equal up to summation rounding: per element at most
 * 2 * gamma_m * sum |t_i| over the m active taps and the bias, gamma_m = m u / (1 - m u), u = 2^-24.
 * Cin <= 16 with a filter bank Cout*Cin*KH*KW*4 <= 64 KiB: the whole bank in LDS (k_conv2d); every other shape: the ordered
 * taps in slabs of 512, 8 output channels per workgroup, the block's images staged channels-last in LDS where they fit 48 KiB
 * (csrc/snn_conv_wide.hip).  Any Cin, Cout, KH, KW, stride >= 1, pad >= 0, B.  SNN_ERR_UNSUPPORTED only where an index leaves
 * its int: Cin*KH*KW > SNN_CONV2D_MAX_TAPS, Cin*H*Wd or OH*OW > SNN_CONV2D_MAX_IMAGE, or more than 2^31 - 1 blocks of 256
 * output pixels (B*OH*OW).                                                                                                  */
#define SNN_CONV2D_MAX_TAPS 0x7fff0000
#define SNN_CONV2D_MAX_IMAGE 0x7fff0000
int snn_prop_conv2d_f32(const float *W, const float *bias, const uint8_t *s, float *out,
                        int B, int Cin, int H, int Wd, int Cout, int KH, int KW,
                        int stride, int pad, int accumulate, snn_stream_t stream);

/* ---- f17: a real-valued (analog) Input layer -------------------------------------------------------
 * The reference's Input.forward is `self.s = x` for any dtype (nodes.py:219) and every compute() starts with `s.float()`: a
 * network may be driven by the real-valued sample itself at every step (encoding.repeat), which is how a network made by
 * bindsnet.conversion is meant to be driven.  An INPUT layer may therefore be fed a FLOAT32 [T,B,n] tensor.  The arithmetic is
 * the stated orders of a6 / a7 / the input step with the spike byte replaced by the real value x, every multiply and every add
 * rounded on its own (-ffp-contract=off); csrc/snn_real.hpp holds the bodies.
 *   Dense   out[b,j] (+)= (...((0 + x[b,0]*W[0,j]) + x[b,1]*W[1,j]) + ...) (+ bias[j]): source index ascending, one rounded
 *           multiply and one rounded add per term, bias (nullable) last, accumulate as in snn_prop_dense_f32.  A kernel may skip a
 *           source whose value is zero for all the samples it handles: the skipped term is +-0, a chain that starts at +0 never
 *           becomes -0, so the result is the same for finite weights (a NaN or an infinite weight at such a source is not seen).
 *   Conv2d  the order of snn_prop_conv2d_f32: one bias-free sequential sum over (kh, kw, cin), input channel innermost,
 *           out-of-image taps skipped, one rounding per multiply and per add, bias last; zero values skipped as above.  Any Cin,
 *           stride >= 1, pad >= 0; the SNN_ERR_UNSUPPORTED limits of snn_prop_conv2d_f32.
 *   Input   s is the caller's slice; x = x * trace_decay, then x = trace_scale where s != 0 (set mode) or x = x + trace_scale * s
 *           (additive: the product rounded, then the add); per-neuron trace_decay / trace_scale through pv as snn_input_step_pv.
 * 0/1 invariance: values that are all 0.0 or 1.0 give, bit for bit, what the same values give as spike bytes through
 * snn_prop_dense_f32 / snn_prop_conv2d_f32 / snn_input_step_pv (x * w is then w or +-0 exactly).
 * snn_prop_dense_real_f32: thread <-> target column, each wave carries the chains of 2 samples (one load of W[i,j] serves the
 * 8 samples of its workgroup), W and the samples' values are staged in LDS chunk by chunk, the skip is per wave.  No split-K, no
 * matrix cores: snn_prop_dense_mfma_f32's equivalence holds for 0/1 operands only.  Limits: Nin < 2^24, B <= 65535.
 * snn_prop_conv2d_real_f32: direct; 8 output channels per thread, their filters in LDS where Cin*KH*KW <= 1024, the block's
 * images in LDS where they fit 48 KiB, else both through L2.  snn_input_step_real_pv: raster_out f32 (nullable), pv nullable,
 * B <= 65535.  (ABI 8, additive)                                                                                            */
int snn_prop_dense_real_f32(const float *W, const float *bias, const float *x, float *out,
                            int B, int Nin, int N, int accumulate, snn_stream_t stream);
int snn_prop_conv2d_real_f32(const float *W, const float *bias, const float *x, float *out,
                             int B, int Cin, int H, int Wd, int Cout, int KH, int KW,
                             int stride, int pad, int accumulate, snn_stream_t stream);
/* (snn_input_step_real_pv is declared behind snn_pervec, next to snn_input_step_pv) */

/* ---- f5: LocalConnection1D / 2D / 3D.compute --------------------------------------------------
 * bindsnet/network/topology.py:1573-1597 (1D), :1731-1746 (2D), :1880-1896 (3D).  s [B, n_src] u8, W [Cin, F*conv_prod,
 * kernel_prod], out [B, F*conv_prod]; src int32 [Cin, conv_prod, kernel_prod] = flat source index of tap k of receptive
 * field o in channel ci (what the class's `unfold` calls gather; one table covers 1D, 2D and 3D).
 * out[b, r] (+)= sum_ci sum_k s[b, src[ci, r % conv_prod, k]] * W[ci, r, k]: the tap sum in ATen's vectorised inner-sum
 * order (snn_normalize_conv2d's order: 8 interleaved lanes of row_sum, leftovers, then the lanes), the channel sum
 * ascending.  accumulate as in snn_prop_cascade_f32.  Event-driven: one sample's spikes are staged in LDS (n_src <= 32768,
 * else read from global memory) and only the taps whose source spiked load their weight.  (ABI 8, additive)           */
int snn_prop_local_f32(const float *W, const int *src, const uint8_t *s, float *out, int B, int Cin, int F,
                       int conv_prod, int kernel_prod, int n_src, int accumulate, snn_stream_t stream);

/* ---- f5: PostPre on a LocalConnection1D / 2D / 3D -------------------------------------------------
 * bindsnet/learning/learning.py:208-389 (+ :87-104).  The reference views its [F*conv_prod, Cin*kernel_prod] update as
 * w.size() = [Cin, F*conv_prod, kernel_prod] -- a raw reinterpretation, restated as it is: W is treated as the flat
 * [F*conv_prod, Cin*kernel_prod] matrix, and element (r, j) pairs target r with the source at flat unfolded position
 * (r % conv_prod)*Cin*kernel_prod + j, decoded as (ci, o, k) and looked up in src.  For Cin = 1 this is the synapse
 * snn_prop_local_f32 reads.  pre = sum_b x_tgt[b,r] * s_src[b,.], post = sum_b s_tgt[b,r] * x_src[b,.] (batch sums in
 * ATen sum(dim=0) order); W -= nu0*pre (nu0 != 0), W += nu1*post (nu1 != 0), W *= decay, clamp.  Every weight is read
 * and written once per call.  (ABI 8, additive)                                                                        */
int snn_local_postpre(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                      const float *x_tgt, int B, int Cin, int F, int conv_prod, int kernel_prod, int n_src,
                      float nu0, float nu1, float decay, int has_min, float wmin, int has_max, float wmax,
                      snn_stream_t stream);

/* ---- f6: Conv1dConnection / Conv3dConnection.compute -----------------------------------------
 * bindsnet/network/topology.py:640-656 (F.conv1d), :979-995 (F.conv3d).  s [B, Cin, D, H, Wd] u8 0/1 spikes, W [Cout, Cin,
 * KD, KH, KW], bias nullable [Cout], out [B, Cout, OD, OH, OW].  Isotropic stride and padding, except that an axis of
 * extent 1 with a kernel of 1 is not padded: a conv1d is D = H = KD = KH = 1.  Dilation 1, Cin <= 16.  Order contract (probed on the reference's torch: conv1d at Cin 1..16, conv3d at Cin 1):
 * per output ONE sequential f32 chain over the taps in ascending (kd, kh, kw), input channel innermost, then + bias;
 * out (+)= that as in snn_prop_conv2d_f32.  Event-driven: a sample's spikes are packed into a channels-last bitstream and
 * only the set bits of each tap row are visited (a silent tap adds +-0).  Filters are staged in LDS where Cin*K <= 12288,
 * else read from L2; the bitstream is staged where n_src <= 131072, else packed where it is read.  (ABI 8, additive)   */
int snn_prop_convnd_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int D, int H,
                        int Wd, int Cout, int KD, int KH, int KW, int stride, int pad, int accumulate,
                        snn_stream_t stream);

/* ---- f6: PostPre on a Conv1dConnection / Conv3dConnection -------------------------------------
 * bindsnet/learning/learning.py:422-455 (conv1d), :499-559 (conv3d), + :87-104.  pp_src int32 [L, J] (J = Cin*K) is the
 * matrix the reference hands to bmm as the source operand (pad + unfold + raw reshape, applied to arange(n_src) + 1),
 * flat source index or -1 for padding; W is its flat [Cout, J] view.  s_src / x_src [B, n_src], s_tgt / x_tgt [B, Cout, L].
 * Order contract: per sample pre = sum_l x_tgt[co,l] * s_src[pp_src[l,j]], post = sum_l s_tgt[co,l] * x_src[pp_src[l,j]],
 * l ascending (torch.bmm at these shapes; every product exact); batch sums in ATen's sum(dim=0) order (one term at B = 1);
 * W -= nu0*pre (nu0 != 0), W += nu1*post (nu1 != 0), W *= decay, clamp.  The post term walks only the spiking target
 * positions.  ws: uint32 [B*Cout*ceil(L/32)] scratch for the packed target spikes, needed (nu1 != 0) only when they exceed
 * 32 KiB of LDS; nullable otherwise.  Every weight is read and written once per call.  (ABI 8, additive)               */
int snn_convnd_postpre(float *W, const int *pp_src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                       const float *x_tgt, int B, int Cout, int L, int J, int n_src, float nu0, float nu1, float decay,
                       int has_min, float wmin, int has_max, float wmax, uint32_t *ws, snn_stream_t stream);

/* ---- a2: Input.forward + Nodes.forward trace ------------------------------------------------
 * bindsnet/network/nodes.py:211-221, :96-107.  s is the caller's input slice (aliased, never
 * copied); x (nullable) is the trace, updated in place; raster_out (nullable) receives s.   */
int snn_input_step(const uint8_t *s, float *x, long n_total, float trace_decay,
                   float trace_scale, int additive, uint8_t *raster_out, snn_stream_t stream);

typedef struct {
    float decay, rest, reset, thresh, refrac, dt;
    int has_lbound; float lbound;
    int traces; float trace_decay, trace_scale; int traces_additive;
} snn_lif_params;

/* ---- a3: LIFNodes.forward -------------------------------------------------------------------
 * bindsnet/network/nodes.py:500-529.  v, refrac [B,N] f32 in/out; s [B,N] u8 out; x nullable
 * trace; I [B,N] input current, masked in place where refractory (nodes.py:511);
 * raster_s / raster_v nullable per-step monitor slices.                                      */
int snn_lif_step(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                 const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v,
                 snn_stream_t stream);
/* The same step with PER-NEURON thresholds (nodes.py:425-498 take `thresh` as a tensor; examples/mnist/reservoir.py builds its
 * LIF layer that way): thresh_vec [N] f32 on the device replaces h_p->thresh, neuron j of every sample compares against
 * thresh_vec[j].  thresh_vec == NULL: snn_lif_step.  (ABI 8)                                                              */
int snn_lif_step_vth(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                     const snn_lif_params *h_p, const float *thresh_vec, uint8_t *raster_s, float *raster_v,
                     snn_stream_t stream);

typedef struct {
    snn_lif_params lif;
    float theta_decay, theta_plus;
    int learning;      /* nodes.py:1078,1093: theta decays / grows only while learning */
    int one_spike;     /* nodes.py:1097 */
} snn_dc_params;

/* ---- f7: McCullochPitts / IFNodes / BoostedLIFNodes / CurrentLIFNodes / IzhikevichNodes.forward --------------------
 * One launch per layer per timestep; every kernel also writes its raster_s / raster_v slice (nullable) and the trace x
 * (nullable unless h_p->traces).  h_p carries the fields the class has (thresh, dt, trace_* always; the rest as listed).
 * Each * and + of the reference is rounded separately (csrc/snn_common.hpp restates the op order).  (ABI 8, additive)
 *
 * snn_mcp_step      bindsnet/network/nodes.py:278-288.  v = I (the mirror keeps its own [B,N] copy), s = v >= thresh.
 * snn_if_step       bindsnet/network/nodes.py:371-395.  v += (refrac <= 0) * I with the gate taken BEFORE the decrement;
 *                   uses reset, refrac, lbound.
 * snn_boosted_step  bindsnet/network/nodes.py:621-648.  v *= decay; I masked in place where refrac > 0 (before the
 *                   decrement); v += I; spiking neurons are reset to the constant 0.  Uses decay, refrac.
 * snn_clif_step     bindsnet/network/nodes.py:762-791.  i [B,N] in/out is the synaptic current: v = decay*(v-rest)+rest,
 *                   i *= i_decay, refrac -= dt, i += I, v += (refrac <= 0) * i with the gate taken AFTER the decrement.
 *                   Uses decay, rest, reset, refrac, lbound.                                                          */
int snn_mcp_step(float *v, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                 uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_if_step(float *v, float *refrac, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_boosted_step(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N, const snn_lif_params *h_p,
                     uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_clif_step(float *v, float *refrac, float *i, uint8_t *s, float *x, const float *I, int B, int N,
                  const snn_lif_params *h_p, float i_decay, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
/* snn_izh_step      bindsnet/network/nodes.py:1265-1296, the whole step in one launch (one workgroup per sample, one thread
 * per neuron).  s [B,N] holds the PREVIOUS step's spikes at entry and this step's at exit.  Where s: v = c, u = u + d.
 * I [B,N] += sum over the spiking neurons i of S[j,i], in the order of ATen's S[:, s[b]].sum(dim=1) (vectorised inner sum
 * over the selected columns in ascending i: csrc/snn_order.hpp inner_sum8_terms); a sample without a spike adds +0.  Then
 * two half-steps v += (dt*0.5) * (0.04*v*v + 5*v + 140 - u + I), u += (dt*a) * (b*v - u), lbound, s = v >= thresh, trace.
 * a, b, c, d: [N].  St: the lateral matrix TRANSPOSED, St[i*N + j] = S[j,i], so that a step reads rows.  Uses thresh, dt,
 * lbound.  Limits: N <= SNN_IZH_MAX_N (the size up to which the summation order is pinned against torch:
 * tests/test_nodes_hostcheck.py), else SNN_ERR_UNSUPPORTED.                                                          */
#define SNN_IZH_MAX_N 1024
int snn_izh_step(float *v, float *u, uint8_t *s, float *x, float *I, const float *a, const float *b, const float *c,
                 const float *d, const float *St, int B, int N, const snn_lif_params *h_p, uint8_t *raster_s,
                 float *raster_v, snn_stream_t stream);

/* ---- f12: SRM0Nodes.forward and Rmax --------------------------------------------------------------
 * bindsnet/network/nodes.py:1639-1671.  The layer's whole step in one launch, the draw included: *rng holds the HOST generator
 * (see snn_rng_state below); element e of the row-major [B,N] range takes its e-th next 32-bit output, u = (r & 0xFFFFFF) * 2^-24
 * -- what torch.rand_like(s_prob) draws -- and *rng is left advanced by B*N outputs (rng->consumed is not touched).  Order:
 * v = decay*(v-rest)+rest;  v += ((refrac <= 0) * eps_0) * I;  rho = rho_0 * exp((v - thresh) / d_thresh);
 * s_prob = 1 - exp(-rho * dt);  refrac -= dt;  s = u < s_prob;  where s: refrac = h_p->refrac, v = reset;  lbound;  trace.
 * s_prob, rho [B,N] f32 out (rho from the voltage BEFORE the reset, as the reference's attribute).  The two exp are the
 * device's expf, a 1-ulp function like torch's: rho and s_prob agree with the reference to a few ulp, everything else to the
 * bit whenever the spikes do.  pv may name thresh, decay, trace_decay, trace_scale.  One workgroup (the stream is serial).
 * (ABI 8, additive)                                                                                                       */
struct snn_rng_state_s;
int snn_srm0_step(struct snn_rng_state_s *rng, float *v, float *refrac, uint8_t *s, float *x, const float *I, float *s_prob,
                  float *rho, int B, int N, const snn_lif_params *h_p, float eps_0, float rho_0, float d_thresh,
                  uint8_t *raster_s, float *raster_v, snn_stream_t stream);
/* bindsnet/learning/learning.py:2923-2960 (+ :87-104), batch 1.  e_trace [Nin,N] in/out, s_tgt / s_prob [N] the target's spikes
 * and spike probabilities of this step, x_src [Nin] the source's (additive) trace.  With k = 1 - dt / tc_e and q = tc_c / dt, both
 * formed in f32:  e = e*k + (s_j - p_j / (1 + q*p_j)) * x_i;  W += (nu0 * reward) * e;  W *= wdecay;  clamp.               */
int snn_rmax_step(float *W, float *e_trace, const uint8_t *s_tgt, const float *s_prob, const float *x_src, int Nin, int N,
                  float reward, float nu0, float dt, float tc_c, float tc_e, float wdecay, int has_min, float wmin,
                  int has_max, float wmax, snn_stream_t stream);

/* ---- f13: CSRMNodes.forward and Connection.compute_window ---------------------------------------------
 * bindsnet/network/nodes.py:1427-1464, topology.py:348-374.  The layer's input is a WINDOW: the last Wres spike vectors of
 * every source, each multiplied by the CURRENT weights.
 * snn_prop_window_f32: ring u8 [B,Wres,Nin] is the connection's window kept as a ring; `head` the physical slot of its oldest
 * entry.  The call overwrites that slot with s [B,Nin] (the push), after which logical slot i (0 = oldest, Wres-1 = s) is
 * physical slot (head + 1 + i) mod Wres, and writes  out[b,i,j] (+)= (((0 + W[s1,j]) + W[s2,j]) + ...) (+ bias[j])  over the
 * sources s1 < s2 < ... that spiked in slot i: ascending source index from 0.0f, one rounded f32 add per term, bias (nullable)
 * last; accumulate as in snn_prop_dense_f32 (0: out = sum, 1: out = out + sum).  out f32 [B,Wres,N].  Event-driven: the work
 * is (spikes in the window) x N, a silent source's row of W is never loaded.  The next call's head is (head + 1) mod Wres.
 * snn_csrm_step, one launch, in this order per (b,j):  v = v * decay;  res = sum_i resK[i] * xwin[b,i,j];  ref = sum_i refK[i]
 * * last[b,i,j]  (both: i ascending from 0.0f, product then add, each one rounding);  v = v + (res + ref);  s = v >= thresh +
 * theta[j]  (theta shared by the batch; while learning it is decayed before the comparison and grows by theta_plus * (the
 * neuron's spike count over the batch) after it, as in snn_dc_step);  last[b] shifted by one slot, s appended;  lbound;  trace.
 * There is no reset and no refractory counter.  pv may name thresh, decay, theta_decay, theta_plus, trace_decay, trace_scale.
 * Limits: Wres, Wref <= SNN_CSRM_MAX_WINDOW, B <= 65535 (snn_prop_window_f32), B*Wres*N, B*Wres*Nin, B*Wref*N < 2^31; beyond
 * them SNN_ERR_UNSUPPORTED.  (ABI 8, additive)                                                                          */
#define SNN_CSRM_MAX_WINDOW 1024
int snn_prop_window_f32(const float *W, const float *bias, uint8_t *ring, int head, const uint8_t *s, float *out,
                        int B, int Wres, int Nin, int N, int accumulate, snn_stream_t stream);
/* (snn_csrm_step takes snn_dc_params and snn_pervec: declared behind them, below) */

/* ---- a4: DiehlAndCookNodes.forward ----------------------------------------------------------
 * bindsnet/network/nodes.py:1069-1111.  theta [N] shared by the batch.  one_spike winner
 * selection reproduces torch.multinomial on the CPU generator: noise_q is the pre-drawn
 * Exp(1) stream (torch.empty(K).exponential_(1)), *cursor (device int64) the number of
 * draws consumed so far; a step with r rows that crossed threshold consumes r*N draws
 * (SURVEY.md Appendix B).  *status (device int32) is set to SNN_ERR_NOISE, and the step
 * leaves s as the un-arbitrated crossings, if fewer than r*N draws remain.                   */
int snn_dc_step(float *v, float *refrac, uint8_t *s, float *x, float *theta, const float *I,
                int B, int N, const snn_dc_params *h_p,
                const float *noise_q, long long q_len, long long *cursor, int *status,
                uint8_t *raster_s, float *raster_v, snn_stream_t stream);

/* The second half of snn_dc_step on its own: bindsnet/network/nodes.py:1097-1111 -- one_spike winner selection on the
 * crossings `s` [B,N] (in: every neuron that crossed its threshold; out: one winner per row that had a crossing), then the
 * trace update with the final spikes (nodes.py:96-107) and the raster slice.  For callers that put something between
 * the membrane update and the arbitration: the exact batch-sharded multi-GPU mode runs the membrane half
 * (snn_dc_step with one_spike = 0, traces = 0, learning = 0) on each rank's rows, gathers the crossings of all ranks, and
 * then arbitrates the GLOBAL batch on every rank, so that the draws are consumed in the global row order.  noise_q /
 * q_len as in snn_dc_step; cursor[1] must hold the offset of this step's first draw inside noise_q
 * (snn_rng_fill_exponential leaves 0 there and the draws in qbuf); cursor[0] receives cursor[1] + rows_with_a_crossing * N.
 * h_p->learning and theta are not used here (the adaptive threshold belongs to the membrane half).           */
int snn_dc_arbitrate(uint8_t *s, float *x, int B, int N, const snn_dc_params *h_p,
                     const float *noise_q, long long q_len, long long *cursor, int *status,
                     uint8_t *raster_s, snn_stream_t stream);

/* ---- f10: per-neuron parameters on every node layer ------------------------------------------
 * bindsnet/network/nodes.py declares most node parameters Union[float, torch.Tensor]; a tensor gives every neuron its own
 * value.  The step kernels read seven per-neuron quantities; each is either the scalar of snn_lif_params / snn_dc_params
 * (or the i_decay argument), or an f32 [N] DEVICE vector indexed by neuron and broadcast over the batch.  snn_pervec holds the
 * vectors: v[q] == NULL means "use the scalar".  The arithmetic is unchanged (csrc/snn_common.hpp): where a vector is given,
 * neuron j's value takes the scalar's place in the same separately rounded operations; the Diehl&Cook threshold bump is
 * theta[j] += theta_plus[j] * count[j], one rounded multiply and one add.  theta_decay[j] applies only while learning.
 * Which quantity a layer kind reads:  thresh: all but INPUT;  decay: LIF, DC, BOOSTED, CURRENT;  trace_decay, trace_scale:
 * every kind (trace_scale only with additive traces: the reference's masked_fill_ takes a 0-dim value);  theta_decay,
 * theta_plus: DC;  i_decay: CURRENT.  A vector the kind does not read is SNN_ERR_INVALID.
 * The *_pv entry points are their scalar namesakes with `pv` (nullable: the scalar step) added; B <= 65535 when pv names a
 * vector (the sample is the launch grid's second dimension, so no kernel divides by N).  (ABI 8, additive)               */
enum { SNN_PV_THRESH = 0, SNN_PV_DECAY = 1, SNN_PV_TRACE_DECAY = 2, SNN_PV_TRACE_SCALE = 3, SNN_PV_THETA_DECAY = 4,
       SNN_PV_THETA_PLUS = 5, SNN_PV_I_DECAY = 6, SNN_PV_COUNT = 7 };
typedef struct { const float *v[SNN_PV_COUNT]; } snn_pervec;

int snn_input_step_pv(const uint8_t *s, float *x, int B, int N, float trace_decay, float trace_scale, int additive,
                      const snn_pervec *pv, uint8_t *raster_out, snn_stream_t stream);
/* f17: the step of a real-valued Input layer (s, raster_out f32).  (ABI 8, additive) */
int snn_input_step_real_pv(const float *s, float *x, int B, int N, float trace_decay, float trace_scale, int additive,
                           const snn_pervec *pv, float *raster_out, snn_stream_t stream);
int snn_lif_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N, const snn_lif_params *h_p,
                    const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_mcp_step_pv(float *v, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                    const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_if_step_pv(float *v, float *refrac, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                   const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_boosted_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N, const snn_lif_params *h_p,
                        const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_clif_step_pv(float *v, float *refrac, float *i, uint8_t *s, float *x, const float *I, int B, int N,
                     const snn_lif_params *h_p, float i_decay, const snn_pervec *pv, uint8_t *raster_s, float *raster_v,
                     snn_stream_t stream);
int snn_izh_step_pv(float *v, float *u, uint8_t *s, float *x, float *I, const float *a, const float *b, const float *c,
                    const float *d, const float *St, int B, int N, const snn_lif_params *h_p, const snn_pervec *pv,
                    uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_dc_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *theta, const float *I, int B, int N,
                   const snn_dc_params *h_p, const snn_pervec *pv, const float *noise_q, long long q_len, long long *cursor,
                   int *status, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_srm0_step_pv(struct snn_rng_state_s *rng, float *v, float *refrac, uint8_t *s, float *x, const float *I, float *s_prob,
                     float *rho, int B, int N, const snn_lif_params *h_p, float eps_0, float rho_0, float d_thresh,
                     const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_csrm_step(float *v, uint8_t *s, float *x, float *theta, const float *xwin, float *last, const float *resK, int Wres,
                  const float *refK, int Wref, int B, int N, const snn_dc_params *h_p, const snn_pervec *pv, uint8_t *raster_s,
                  float *raster_v, snn_stream_t stream);

/* ---- f14: bindsnet.conversion -- SubtractiveResetIFNodes, PassThroughNodes, PermuteConnection, ConstantPad2dConnection ----
 * snn_sif_step      bindsnet/conversion/nodes.py:73-99, one launch, state streamed once.  Per element, every operation one
 *                   rounded f32 operation:  v += float(refrac == 0) * I;  refrac = float(refrac > 0) * (refrac - dt);
 *                   s = v >= thresh;  where s: refrac = h_p->refrac, v = v - thresh (reset by subtraction: `reset` is only
 *                   the value reset_state_variables() fills in);  lbound;  trace;  summed += I (the raw input; `summed`
 *                   f32 [B,N] nullable -- Nodes(sum_input=True) -- and free when NULL: a kernel instance of its own).
 *                   Uses thresh, refrac, dt, lbound and the trace fields.  pv (the _pv form) may name trace_decay and
 *                   trace_scale only: the reference's `v[s] - thresh` cannot broadcast a tensor-valued threshold either.
 * snn_pass_step     bindsnet/conversion/nodes.py:161-169: s = I, kept as a spike byte (I != 0; what feeds such a layer
 *                   emits 0.0 or 1.0), plus the raster_s slice.  No voltage, no trace, no summed.
 * snn_prop_gather_f32  PermuteConnection.compute (`s.permute(dims).float()`, dims[0] == 0) and ConstantPad2dConnection
 *                   .compute (`F.pad(s, padding).float()`, fill 0) as one gather: out f32 [B, out[0], out[1], out[2]],
 *                   s spike bytes [B, n_src];  out[b, i0, i1, i2] (+)= float(s[b, sum_a (i_a - off[a]) * stride[a]]) where
 *                   every i_a - off[a] lies in [0, src[a]), else (+)= 0.  out / src / stride / off are HOST arrays of three
 *                   ints (missing leading dimensions: extent 1, stride 0, offset 0); there is no index table.  A geometry
 *                   that could read outside [0, n_src) or that crops (off[a] + src[a] > out[a]) is SNN_ERR_INVALID.
 *                   accumulate as snn_prop_pool_f32.  (ABI 8, additive)                                                    */
int snn_sif_step(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, int B, int N,
                 const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_sif_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, int B, int N,
                    const snn_lif_params *h_p, const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
int snn_pass_step(uint8_t *s, const float *I, int B, int N, uint8_t *raster_s, snn_stream_t stream);
int snn_prop_gather_f32(const uint8_t *s, float *out, int B, int n_src, const int *out_ext, const int *src_ext,
                        const int *stride, const int *off, int accumulate, snn_stream_t stream);

/* ---- f18: AvgPool2dConnection.compute ---------------------------------------------------------------
 * Not in the reference (an extension for converted networks); the oracle is ATen's avg_pool2d on the CPU:
 *   out (+)= F.avg_pool2d(float(s), k, stride, pad, ceil_mode, count_include_pad, divisor_override)
 * s spike bytes [B, C, in[0], in[1]] (a non-zero byte counts as one spike), out f32 [B, C, out[0], out[1]] with
 * out[a] = floor((in[a] + 2 pad[a] - k[a] + (ceil_mode ? stride[a] - 1 : 0)) / stride[a]) + 1, less one with ceil_mode where the
 * last window would start at or behind in[a] + pad[a].  Per output: the window is clipped to the padded plane (the product of
 * the two lengths is pool_size), then to the plane; the spikes inside are COUNTED as an integer; the value is
 * f32(count) / f32(divisor), one correctly rounded division, with divisor = divisor_override where that is non-zero, else
 * pool_size (count_include_pad) or the number of in-plane taps; a window without an in-plane tap gives 0.  accumulate adds the
 * value onto out with one rounded add, as snn_prop_local_f32.  Integer counts make every summation order give the same bits:
 * windows of fewer than SNN_AVGPOOL_COOP_TAPS taps (k[0] * k[1]) take one thread per output, larger ones one wave per output
 * (csrc/snn_avgpool.hip), on at most SNN_AVGPOOL_MAX_GRID workgroups of SNN_AVGPOOL_THREADS threads striding over the outputs.
 * in / k / stride / pad are HOST arrays of two ints.  2 * pad[a] > k[a] (torch refuses it), an empty output, k[0] * k[1] beyond
 * 2^24 or a plane beyond 2^30 elements is SNN_ERR_INVALID; B * C beyond 2^30 or more than 2^40 elements SNN_ERR_UNSUPPORTED.
 * snn_set_avgpool_body: 0 -- the rule above (the default); 1 / 2 -- the per-thread / the per-wave body for every geometry
 * (tests and measurements: the crossover, profiles/NOTES_avgpool.md).  (ABI 8, additive)                                  */
#define SNN_AVGPOOL_COOP_TAPS 64
#define SNN_AVGPOOL_THREADS 256
#define SNN_AVGPOOL_MAX_GRID 1024
int snn_prop_avgpool2d_f32(const uint8_t *s, float *out, int B, int C, const int *in, const int *k, const int *stride,
                           const int *pad, int ceil_mode, int count_include_pad, int divisor_override, int accumulate,
                           snn_stream_t stream);
void snn_set_avgpool_body(int body);

/* ---- device-resident emulation of torch's CPU generator --------------------------------------
 * Replaces the pre-drawn noise_q stream: the library reproduces the draws torch.multinomial
 * (bindsnet/network/nodes.py:1100-1102) would consume -- mt19937 -> random64 -> u in [0,1) ->
 * (float)(-log1p(-u)) -- on the device, bit-exactly, from the generator state the host uploads
 * (parsed from torch.get_rng_state()).  pos: index of the next output inside the current 624-word
 * block, 624 = "twist before the next output" (at::mt19937's left_ == 1).  consumed counts draws.
 * After the run the host downloads the struct and writes it back with torch.set_rng_state(). */
typedef struct snn_rng_state_s {
    uint32_t mt[624];
    int32_t pos;
    int32_t reserved;
    long long consumed;
} snn_rng_state;

/* For the rows of `crossings` [B,N] that contain a non-zero entry (r of them, in row order) write
 * the draws of the [r, N] operand's candidate positions to qbuf[rank*N + j], advance *rng by r*N
 * draws and zero cursor[1], so that snn_dc_step-style arbitration can index qbuf from 0.      */
int snn_rng_fill_exponential(snn_rng_state *rng, const uint8_t *crossings, int B, int N, float *qbuf,
                             long long *cursor, snn_stream_t stream);

/* ---- a8 / a9: PostPre -----------------------------------------------------------------------
 * MCC: bindsnet/learning/MCC_learning.py:224-302 + :86-110 (use_dt = 1: each reduced update
 * is multiplied by connection.dt).  Dense: bindsnet/learning/learning.py:390-420 + :87-104
 * (use_dt = 0).  W -= sum_b s_src (x) (x_tgt*nu0); W += sum_b x_src (x) (s_tgt*nu1);
 * W *= decay; clamp.  Batch sums in ATen sum(dim=0) order.  nu0 == 0 / nu1 == 0 skip that
 * half like the reference.  assume_clamped = 1: the caller guarantees decay == 1 and W already
 * inside [wmin, wmax], so elements with no pre- and no post-synaptic spike are skipped.
 * Limits: B <= 256.                                                                          */
int snn_stdp_postpre(float *W, const uint8_t *s_src, const float *x_src,
                     const uint8_t *s_tgt, const float *x_tgt, int B, int Nin, int N,
                     float nu0, float nu1, int use_dt, float dt, float decay,
                     int has_min, float wmin, int has_max, float wmax, int assume_clamped,
                     snn_stream_t stream);

/* ---- a10: MSTDP -----------------------------------------------------------------------------
 * bindsnet/learning/learning.py:1504-1574.  The reference's dense eligibility [B,Nin,N] is kept
 * FACTORED: elig[b] = p_plus[b] (x) s_tgt_prev[b] + s_src_prev[b] (x) p_minus[b], where p_plus /
 * p_minus are the values left by the previous call and *_prev the spikes of the previous call
 * (in/out, zero before the first call == the reference's zero-initialised eligibility).
 * Order: W += nu0 * sum_b reward*elig[b]  (batch sum in ATen sum(dim=0) order);
 *        p_plus = p_plus*decay_plus + a_plus*s_src;  p_minus = p_minus*decay_minus + a_minus*s_tgt;
 *        *_prev = current spikes;  W *= wdecay;  clamp.
 * reward_vec (nullable, device [B]) overrides the scalar reward.  Limits: B <= 256.          */
int snn_mstdp_step(float *W, float *p_plus, float *p_minus,
                   uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                   const uint8_t *s_src, const uint8_t *s_tgt, int B, int Nin, int N,
                   float reward, const float *reward_vec, float nu0, float a_plus, float a_minus,
                   float decay_plus, float decay_minus, float wdecay,
                   int has_min, float wmin, int has_max, float wmax, snn_stream_t stream);

/* ---- f3: Hebbian / WeightDependentPostPre (dense Connection) --------------------------------------
 * bindsnet/learning/learning.py:1110-1135 and :626-653 (+ LearningRule.update :87-104).  U1 = sum_b s_src (x) x_tgt,
 * U2 = sum_b x_src (x) s_tgt (ATen batch-sum order), then
 *   weight_dependent = 0:  W += nu0 * U1;  W += nu1 * U2
 *   weight_dependent = 1:  update = 0 - (nu0 U1)(W - wmin) + (nu1 U2)(wmax - W);  W += update   (needs both bounds)
 * followed by W *= decay and the clamp.  Limits: B <= 256.                                              */
int snn_stdp_hebbian(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                     int B, int Nin, int N, float nu0, float nu1, int weight_dependent, float decay,
                     int has_min, float wmin, int has_max, float wmax, snn_stream_t stream);

/* ---- f4: PostPre on a Conv2dConnection -----------------------------------------------------------------
 * bindsnet/learning/learning.py:457-497 (+ :87-104).  With k = (cin,kh,kw), l = (oy,ox) and unfold = im2col:
 *   W[co,k] -= nu0 * sum_b sum_l x_tgt[b,co,l] * unfold(s_src)[b,k,l];  W[co,k] += nu1 * sum_b sum_l s_tgt[b,co,l] *
 *   unfold(x_src)[b,k,l];  W *= decay; clamp.  The sum over l is sequential in ascending l (the reference's runs inside
 * torch.bmm: BLAS order, compared within tolerance), the batch sum in ATen's sum(dim=0) order.
 * ws: device scratch of 2 * B * Cout*Cin*KH*KW floats.                                                       */
int snn_conv2d_postpre(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                       int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                       float decay, int has_min, float wmin, int has_max, float wmax, float *ws, snn_stream_t stream);

/* ---- f4: Hebbian / WeightDependentPostPre on a Conv2dConnection --------------------------------------------
 * bindsnet/learning/learning.py:1348-1380 and :920-976 (+ :87-104).  pre[co,k] = sum_b sum_l x_tgt[b,co,l] * unfold(s_src)[b,k,l] and
 * post[co,k] = sum_b sum_l s_tgt[b,co,l] * unfold(x_src)[b,k,l] are snn_conv2d_postpre's two sums (same kernels, same order), then
 *   weight_dependent = 0:  W += nu0 * pre;  W += nu1 * post              (both statements always run)
 *   weight_dependent = 1:  u = 0;  nu0 != 0: u = u - (nu0 pre)(W - wmin);  nu1 != 0: u = u + (nu1 post)(wmax - W);  W += u
 *                          (needs both bounds: SNN_ERR_INVALID without)
 * followed by W *= decay and the clamp; every operation rounds once.  ws: device scratch of 2 * B * Cout*Cin*KH*KW floats. */
int snn_conv2d_hebbian(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                       int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                       int weight_dependent, float decay, int has_min, float wmin, int has_max, float wmax, float *ws,
                       snn_stream_t stream);

/* ---- f4: MSTDP on a Conv2dConnection (batch 1) -----------------------------------------------------------
 * bindsnet/learning/learning.py:1942-2015 (+ :87-104), defined at batch size 1 only (the reference views its [B, Cout, K]
 * eligibility as the weight's shape, :2013).  elig [Cout, K = Cin*KH*KW] is the rule's eligibility (in/out), p_plus the
 * P^+ trace in input space [Cin, H, W] (the reference's unfolded copy carries the same values), p_minus P^- [Cout, OH*OW].
 * Order:  W[co,k] += nu0 * sum_co' (reward * elig[co',k])  (the reference's torch.sum(update, dim=0) over a weight-shaped
 * eligibility: summed over the OUTPUT CHANNELS in ATen's order and broadcast back, :1966-1967);  W *= wdecay; clamp;
 * p_plus = p_plus * decay_plus + a_plus * s_src;  p_minus likewise with s_tgt;
 * elig[co,k] = sum_l s_tgt[co,l] * unfold(p_plus)[k,l] + sum_l p_minus[co,l] * unfold(s_src)[k,l]  (each ascending in l; the
 * reference's run inside torch.bmm: BLAS order, compared within tolerance).                                       */
int snn_conv2d_mstdp_step(float *W, float *elig, float *p_plus, float *p_minus, const uint8_t *s_src, const uint8_t *s_tgt,
                          int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float reward, float nu0,
                          float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min,
                          float wmin, int has_max, float wmax, snn_stream_t stream);

/* ---- f3: MSTDPET (dense Connection, batch 1) -----------------------------------------------------------
 * bindsnet/learning/learning.py:2187-2248.  e_trace [Nin,N] is the rule's dense eligibility trace (in/out); the point
 * eligibility is p_plus (x) s_tgt_prev + s_src_prev (x) p_minus of the previous call's factors, formed on the fly.
 * Order: e_trace = e_trace * decay_e + elig / tc_e;  W += ((nu0 * dt) * reward) * e_trace;  W *= wdecay; clamp;
 * then p_plus / p_minus / *_prev advance as in snn_mstdp_step.                                           */
int snn_mstdpet_step(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                     const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt,
                     float a_plus, float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e,
                     float wdecay, int has_min, float wmin, int has_max, float wmax, snn_stream_t stream);

/* ---- a11: normalize -------------------------------------------------------------------------
 * AbstractFeature.normalize, bindsnet/network/topology_features.py:250-266 (use_abs = 0) and
 * Connection.normalize, bindsnet/network/topology.py:383-392 (use_abs = 1).
 * colsum in ATen sum(dim=0) order, zero -> 1, W *= norm * (1/colsum).
 * colsum_ws: device scratch of N floats.                                                      */
int snn_normalize(float *W, int Nin, int N, float norm, int use_abs, float *colsum_ws,
                  snn_stream_t stream);

/* Conv2dConnection.normalize, bindsnet/network/topology.py:824-837: W viewed as [n_filters = Cout*Cin, taps = KH*KW]; every filter is
 * scaled to sum `norm` -- w[f] *= norm * (1 / sum_k w[f,k]), the sum in ATen's vectorised inner-sum order (8 interleaved lanes of
 * row_sum, leftovers, then the lanes), no zero guard like the reference.  (ABI 6)                                  */
int snn_normalize_conv2d(float *W, int n_filters, int taps, float norm, snn_stream_t stream);

/* ---- f12: float16 / bfloat16 Weight features --------------------------------------------------
 * A MulticompartmentConnection whose single Weight has value_dtype torch.float16 or torch.bfloat16 (w_dtype 1 / 2, SNN_W_*): W is
 * the [Nin, N] value as 2-byte elements; neuron state, traces and currents stay f32.  All arithmetic is f32 on exactly widened
 * values, with one round-to-nearest-even conversion to the weight dtype ("->h", overflow to +-inf) where the reference stores
 * into or produces a tensor of that dtype (csrc/snn_half.hpp):
 *   snn_prop_cascade_h16   snn_prop_cascade_f32's sum over the widened weights, ->h, widened, stored (0 + r) or added to out;
 *   snn_stdp_postpre_h16   MCC_learning.py:224-302 + :86-110: w = (w - pre*dt)->h if nu0 != 0; w = (w + post*dt)->h if
 *                          nu1 != 0; w = (w * decay)->h; clamp.  pre / post: f32 batch sums (B = 1: squeeze).  Limits: B <= 256;
 *   snn_normalize_h16      topology_features.py:250-266: cs = colsum->h (0 -> 1), r = (1/cs)->h, f = (r*norm)->h, w = (w*f)->h;
 *                          colsum_ws: device scratch of N floats.
 * Spike bytes are 0 or 1.  Added without changing SNN_ABI_VERSION: purely additive.                              */
enum { SNN_W_F32 = 0, SNN_W_F16 = 1, SNN_W_BF16 = 2 };
int snn_prop_cascade_h16(const void *W, int w_dtype, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                         snn_stream_t stream);
int snn_stdp_postpre_h16(void *W, int w_dtype, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                         const float *x_tgt, int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay,
                         int has_min, float wmin, int has_max, float wmax, snn_stream_t stream);
int snn_normalize_h16(void *W, int w_dtype, int Nin, int N, float norm, float *colsum_ws, snn_stream_t stream);

/* ---- f13: per-synapse learning rates and weight bounds, per-target norms --------------------------
 * The reference takes `nu` as a pair of tensors (learning.py:44-46, :67), `wmin` / `wmax` as tensors of the weights' size
 * (topology.py:49-52; `range` of a Weight, MCC_learning.py:52) and `norm` as one total per target neuron
 * (topology_features.py:207-208).  snn_synparams names those constants: each pointer is a device f32 array read as
 * p[s * rs + n * cs] for the weight element (source s, target n), with element strides rs, cs (0 on a broadcast axis, so a [N]
 * vector stays a [N] vector in memory); a NULL pointer leaves the constant to the entry point's scalar argument.  nu0_any /
 * nu1_any: whether ANY entry of the rate tensor is non-zero -- the reference's `self.nu[i].any()` (learning.py:399, :409, :642,
 * :647), which decides whether the half of the update runs at all; with it set, elements whose own rate is 0 still go through the
 * arithmetic (w - 0, like the reference).  The *_pv entry points compute what their scalar namesakes compute, every element with
 * its own constants: the products with the rates sit where they sit there (`x_tgt * nu0`, `nu * U`, `(nu * U) * (w - wmin)`,
 * `((nu0 * dt) * reward) * e`), the clamp is min(max(w, wmin), wmax) with an absent bound as -inf / +inf.  A NULL `sp`, or one
 * whose four pointers are NULL, is the scalar entry point.  The pair (rs, cs) must be that of a shape that broadcasts against [Nin, N] -- (0, 0) one
 * element, (0, 1) [N] or [1, N], (1, 0) [S, 1], (N, 1) [S, N]; a size-1 axis has stride 0 --, anything else: SNN_ERR_INVALID.
 *   snn_stdp_postpre_pv   learning.py:390-420 / MCC_learning.py:224-302: the rates multiply the [B, N] target factors, so they
 *                         must not vary along the source axis (nu*_rs == 0; the reference's bmm fails on anything else, :401-402).
 *                         assume_clamped keeps its meaning: the bounds of an element do not change within a run.
 *   snn_stdp_hebbian_pv   learning.py:1110-1135 / :626-653 (weight_dependent: every element needs finite bounds, the caller's duty).
 *   snn_mstdp_step_pv     learning.py:1504-1574, :1561 `w += nu[0] * update`.
 *   snn_mstdpet_step_pv   learning.py:2187-2248, :2232 `nu[0] * dt * reward * eligibility_trace`.
 *   snn_normalize_pv      topology.py:383-392 / topology_features.py:250-266 with a tensor norm: scale[n] = norm_vec[n] / colsum[n], ONE
 *                         IEEE division (a python-float norm is reciprocal-then-multiply in ATen: snn_normalize), then one multiply
 *                         per weight.  norm_vec: device [N].  Column sums and the zero -> 1 guard as in snn_normalize.
 * Added without changing SNN_ABI_VERSION: purely additive.                                                        */
typedef struct snn_synparams {
    const float *nu0, *nu1, *wmin, *wmax;
    int nu0_rs, nu0_cs, nu1_rs, nu1_cs, wmin_rs, wmin_cs, wmax_rs, wmax_cs;
    int nu0_any, nu1_any;
} snn_synparams;
int snn_stdp_postpre_pv(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                        int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin, int has_max,
                        float wmax, int assume_clamped, const snn_synparams *sp, snn_stream_t stream);
int snn_stdp_hebbian_pv(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                        int N, float nu0, float nu1, int weight_dependent, float decay, int has_min, float wmin, int has_max,
                        float wmax, const snn_synparams *sp, snn_stream_t stream);
int snn_mstdp_step_pv(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                      const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0, float a_plus,
                      float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin, int has_max,
                      float wmax, const snn_synparams *sp, snn_stream_t stream);
int snn_mstdpet_step_pv(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                        const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt, float a_plus,
                        float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e, float wdecay, int has_min,
                        float wmin, int has_max, float wmax, const snn_synparams *sp, snn_stream_t stream);
int snn_normalize_pv(float *W, int Nin, int N, const float *norm_vec, int use_abs, float *colsum_ws, snn_stream_t stream);

/* ---- f16: Weight(norm_frequency="time step") -- propagation and normalisation of one Weight in one launch --------
 * bindsnet/network/topology_features.py:633-645: Weight.compute forms value * conn_spikes and then, in "time step" mode, normalises
 * the value in place (:250-266, signed column sums).  out[b, j] (+)= sum_i W[i, j] * s[b, i] from the weights AS THEY WERE, in
 * snn_prop_cascade_f32's order (accumulate as there); then every column of W is scaled and written back once.
 * Contract: bit-identical, in `out` and in `W`, to snn_prop_cascade_f32 followed by snn_normalize(use_abs 0) -- the _pv form:
 * snn_normalize_pv(use_abs 0), norm_vec device [N] -- with the same argument checks.  A workgroup keeps 16 columns with all their
 * rows in LDS (csrc/snn_normstep.hip); where that tile does not fit (Nin above about 1100) the entry point makes the two calls
 * itself, through colsum_ws ([N] floats, always required).  Added without changing SNN_ABI_VERSION: purely additive. */
int snn_prop_cascade_norm_f32(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate, float norm,
                              float *colsum_ws, snn_stream_t stream);
int snn_prop_cascade_norm_pv_f32(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                                 const float *norm_vec, float *colsum_ws, snn_stream_t stream);

/* ---- f14: time-averaged updates of the MulticompartmentConnection rules (average_update / continues_update) -----
 * bindsnet/learning/MCC_learning.py:211-222, :237-289 (PostPre), :457-466, :518-535 (MSTDP), :641-649, :696-713 (MSTDPET).  With
 * average_update = K a rule stores each step's update in slot `idx` of a ring of K weight-shaped slots (f32 [K, Nin, N], caller-owned,
 * never cleared by the rule) and, when due, applies torch.mean(ring, dim=0): ATen's sum(dim=0) over the [K, Nin*N] ring in its own
 * order (the batch reduction's, csrc/snn_order.hpp batch_sum, with K terms), then one division by K.  `idx` is the ring index at the
 * START of the step (the caller advances it by one per call, mod K); due = `continuous` (continues_update), or idx + 1 == K (the step
 * in which the index wraps).  The slot is written for every element, zeros included.  Decay and clamp run every step.
 *   snn_postpre_avg_step   pre (nu0 != 0):  ring_pre[idx_pre] = reduce_b s_src * (x_tgt * nu0);  due: W -= mean(ring_pre) * dt;
 *                          post (nu1 != 0): ring_post[idx_post] = reduce_b x_src * (s_tgt * nu1); due: W += mean(ring_post) * dt;
 *                          W *= decay; clamp.  A term whose rate is 0 does not run: the caller leaves its index alone.
 *   snn_mstdp_avg_step     ring[idx] = reduce_b reward * elig_prev[b] (no nu);  due: W += nu0 * mean(ring);  W *= wdecay; clamp;
 *                          then p_plus / p_minus / *_prev advance as in snn_mstdp_step.
 *   snn_mstdpet_avg_step   e_trace as in snn_mstdpet_step;  ring[idx] = ((nu0 * dt) * reward) * e_trace;  due: W += mean(ring);
 *                          W *= wdecay; clamp;  then the factors advance.  Batch 1.
 * reduce_b: ATen's sum(dim=0) over the batch (every shape class of batch_sum, Nin*N == 1 and 4..7 included), or with `squeeze`
 * (batch 1, reduction = torch.squeeze) the product itself.  Limits: K <= 256 and B <= 256 (SNN_ERR_UNSUPPORTED beyond); scalar
 * rates and bounds only.  One launch per call for the weights and the rings, one more for the factors of the reward rules.
 * Added without changing SNN_ABI_VERSION: purely additive.                                                          */
#define SNN_AVG_MAX_TERMS 256
int snn_postpre_avg_step(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                         int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max, float wmax,
                         int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre, int idx_post,
                         snn_stream_t stream);
int snn_mstdp_avg_step(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                       const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0, float a_plus,
                       float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin, int has_max,
                       float wmax, int squeeze, float *ring, int K, int continuous, int idx, snn_stream_t stream);
int snn_mstdpet_avg_step(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                         const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt, float a_plus,
                         float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e, float wdecay, int has_min,
                         float wmin, int has_max, float wmax, float *ring, int K, int continuous, int idx, snn_stream_t stream);

/* ---- f15: batch reductions beside sum (reduction = torch.mean / torch.amax / torch.amin) -----------------------------
 * Every learning rule of the reference folds the per-sample terms T[b, e] of a batch with `self.reduction(T, dim=0)`
 * (learning.py:76-82, MCC_learning.py:75-81).  The *_red entry points compute what their namesakes compute with that fold chosen by
 * `reduce`; the reduction sits where the reference has it, BEFORE nu / dt / the weight-dependent factors wherever the namesake applies
 * those to the sum, and with the rate inside the terms where the namesake has it there (PostPre on dense and MCC connections).
 *   SNN_REDUCE_SUM   the namesake itself (the call is forwarded).
 *   SNN_REDUCE_MEAN  ATen's sum(dim=0) in the namesake's order, then ONE correctly rounded f32 division by B -- the bits of torch.mean
 *                    on one thread; never a multiplication by 1/B.
 *   SNN_REDUCE_AMAX  the maximum over all B terms.  The event-driven kernels visit only the samples with a spike on the element's
 *   SNN_REDUCE_AMIN  source or target; every other sample is a zero term, so 0.0f is folded in whenever fewer than B were visited.
 *                    The SIGN of a zero result is not defined (torch.amax of a column holding +0 and -0 differs between its scalar
 *                    and vector paths); it never reaches a value: w + (+-0), clamp and normalize give the same weights.
 *                    A NaN term makes the result NaN, as torch.amax / torch.amin propagate it.
 * A `reduce` outside the enum is SNN_ERR_INVALID.  `sp` as in the *_pv entry points (NULL: scalar rates and bounds); the dense
 * family runs these reductions through the per-synapse kernel's tiles with the accumulator exchanged, scalars included.  `squeeze`
 * (batch 1) keeps its meaning where it exists; at B == 1 every reduction is the identity.  MSTDPET and MSTDP on a Conv2dConnection
 * hard-code torch.sum in the reference (batch 1) and have no *_red form; Rmax has no reduction.
 * Added without changing SNN_ABI_VERSION: purely additive.                                                          */
enum { SNN_REDUCE_SUM = 0, SNN_REDUCE_MEAN = 1, SNN_REDUCE_AMAX = 2, SNN_REDUCE_AMIN = 3 };
int snn_stdp_postpre_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                         int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin, int has_max,
                         float wmax, int assume_clamped, const snn_synparams *sp, int reduce, snn_stream_t stream);
int snn_stdp_hebbian_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                         int N, float nu0, float nu1, int weight_dependent, float decay, int has_min, float wmin, int has_max,
                         float wmax, const snn_synparams *sp, int reduce, snn_stream_t stream);
int snn_mstdp_step_red(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                       const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0, float a_plus,
                       float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin, int has_max,
                       float wmax, const snn_synparams *sp, int reduce, snn_stream_t stream);
int snn_conv2d_postpre_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Cin,
                           int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1, float decay,
                           int has_min, float wmin, int has_max, float wmax, float *ws, int reduce, snn_stream_t stream);
int snn_conv2d_hebbian_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Cin,
                           int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1, int weight_dependent,
                           float decay, int has_min, float wmin, int has_max, float wmax, float *ws, int reduce, snn_stream_t stream);
int snn_local_postpre_red(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                          int B, int Cin, int F, int conv_prod, int kernel_prod, int n_src, float nu0, float nu1, float decay,
                          int has_min, float wmin, int has_max, float wmax, int reduce, snn_stream_t stream);
int snn_convnd_postpre_red(float *W, const int *pp_src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                           const float *x_tgt, int B, int Cout, int L, int J, int n_src, float nu0, float nu1, float decay,
                           int has_min, float wmin, int has_max, float wmax, uint32_t *ws, int reduce, snn_stream_t stream);
int snn_stdp_postpre_h16_red(void *W, int w_dtype, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                             int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin,
                             int has_max, float wmax, int reduce, snn_stream_t stream);
/* The reduced update is what goes into the ring slot (MCC_learning.py:238, :275, :519); the ring's own mean is unchanged. */
int snn_postpre_avg_step_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                             int Nin, int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max,
                             float wmax, int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre,
                             int idx_post, int reduce, snn_stream_t stream);
int snn_mstdp_avg_step_red(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                           const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                           float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                           int has_max, float wmax, int squeeze, float *ring, int K, int continuous, int idx, int reduce,
                           snn_stream_t stream);

/* ---- f2: spike encoders on the device ---------------------------------------------------------
 * bindsnet/encoding/encodings.py:51-98 (bernoulli): out [steps, n] u8 = what torch.bernoulli(max_prob *
 * datum.repeat([steps, 1])) draws from the HOST generator whose state is in *rng -- one 32-bit mt19937 output
 * per element, u = (r & 0xFFFFFF) * 2^-24 < p -- bit for bit; *rng is advanced by steps * n outputs.
 * bindsnet/encoding/encodings.py:101-152 (poisson): same construction (intervals ~ Poisson(1000 / (x dt)), zeros
 * bumped to one, cumulated) from a Philox-4x32-10 stream keyed by (seed, element): same distribution, NOT the reference's
 * stream (ATen's sampler draws a data-dependent number of outputs per element).  The stream is SPECIFIED operation by
 * operation (csrc/snn_encode.hip: IEEE f32 / f64 adds, multiplies, divides, f32 sqrt, integer conversions; exp / log /
 * log k! are fixed series, no libm) and restated in oracle/snn_oracle.c (orc_encode_poisson), bit for bit.  out is
 * written completely (zeroed, then the spikes).                                                        */
int snn_encode_bernoulli(snn_rng_state *rng, const float *datum, int n, int steps, float max_prob, uint8_t *out,
                         snn_stream_t stream);
int snn_encode_poisson(const float *datum, int n, int steps, float dt, unsigned long long seed, uint8_t *out,
                       snn_stream_t stream);

/* ---- f8: the Bernoulli mask of a Probability feature ---------------------------------------------
 * bindsnet/network/topology_features.py:425-429: what ONE torch.bernoulli(value) of an [S, N] value draws from the HOST
 * generator whose state is in *rng -- S*N consecutive 32-bit outputs in row-major order, u = (r & 0xFFFFFF) * 2^-24 < p, the
 * stream of snn_encode_bernoulli -- written as bits: bits is uint32 [S, ceil(N/32)], bit (j & 31) of word [i, j >> 5] is
 * element (i, j), the padding bits of a row are 0.  p_scalar != 0: p has one element.  *rng is advanced by S*N outputs; the
 * partially consumed 624-word block carries over to the next call, whoever makes it.  One workgroup (the stream is serial). */
int snn_mcc_bernoulli(snn_rng_state *rng, const float *p, int p_scalar, int S, int N, uint32_t *bits, snn_stream_t stream);

/* ---- Network.reset_state_variables ----------------------------------------------------------
 * bindsnet/network/network.py:467-481 (-> nodes.py:109-120, :531-538, :1113-1120): spikes, traces and
 * refractory counters <- 0, voltages <- rest.  One launch fills up to SNN_MAX_FILL_SEGMENTS device buffers:
 * `pattern` is the 32-bit word every aligned word of the buffer receives (0, or the bit pattern of the f32
 * rest potential; a non-zero pattern needs a 4-byte aligned buffer of a multiple of 4 bytes).         */
#define SNN_MAX_FILL_SEGMENTS 32
typedef struct { void *ptr; unsigned long long bytes; uint32_t pattern; } snn_fill_segment;
int snn_fill_segments(const snn_fill_segment *h_segs, int n, snn_stream_t stream);

/* ---- Monitor.record for float state (x, theta, refrac_count, i, a connection's activity) -----
 * bindsnet/network/monitors.py:94-111, called at the end of every timestep (network.py:459-461): record() clones whatever
 * attribute it is given.  Here the [T, ...] recording is one device buffer per monitored tensor, and timestep t copies
 * segment k's `bytes` bytes from `src` to `dst + t * bytes` -- all n segments in one launch per group of at most
 * SNN_MAX_RECORD_SEGMENTS (the table travels by value in the kernel arguments: no host synchronisation, no staging copy).
 * A plain copy of 32-bit words: the sign of zero and NaN payloads survive.  A segment whose source and destination slice are
 * both 16-byte aligned moves 16 bytes per lane, any other (a theta of odd length beyond t = 0, a view that starts one float
 * into a buffer) 4 bytes per lane.  SNN_ERR_INVALID, before anything is launched: n < 0, t < 0, a NULL table with n > 0, a
 * NULL or not 4-byte aligned pointer in a non-empty segment, `bytes` not a multiple of 4.  Empty segments are skipped.
 * Source and destination slice of a segment must not overlap.  Added without changing SNN_ABI_VERSION: purely additive. */
#define SNN_MAX_RECORD_SEGMENTS 32
typedef struct { const void *src; void *dst; unsigned long long bytes; } snn_record_segment;
int snn_record_segments(const snn_record_segment *h_segs, int n, long long t, snn_stream_t stream);

/* ---- a1: Network.run ------------------------------------------------------------------------
 * bindsnet/network/network.py:380-465 (the per-timestep loop and the post-loop normalisation),
 * for graphs built from {Input, LIFNodes, DiehlAndCookNodes / AdaptiveLIFNodes, McCullochPitts, IFNodes, BoostedLIFNodes,
 * CurrentLIFNodes, IzhikevichNodes, SRM0Nodes, CSRMNodes, SubtractiveResetIFNodes, PassThroughNodes} x {MulticompartmentConnection+Weight,
 * Connection, SparseConnection, Conv1d / Conv2d / Conv3dConnection, LocalConnection1D / 2D / 3D, MaxPool1d / 2d / 3dConnection,
 * MeanFieldConnection, PermuteConnection, ConstantPad2dConnection} x {no rule, PostPre, MSTDP, ...}.  The fused plans match Input / LIF / DC graphs only; a graph
 * with any other layer kind runs the generic plan.  The descriptors are HOST
 * structs holding DEVICE pointers; layers and connections are listed in network insertion
 * order, which fixes the evaluation order exactly as the reference's dict iteration does.   */
/* SNN_LAYER_MCP .. SNN_LAYER_IZH (nodes.py:231, :308, :562, :681, :1147; generic plan only) and the aux / izh_* fields at the
 * end of snn_layer_desc were added without changing SNN_ABI_VERSION, like the additive connection kinds below.  */
enum { SNN_LAYER_INPUT = 0, SNN_LAYER_LIF = 1, SNN_LAYER_DC = 2, SNN_LAYER_MCP = 3, SNN_LAYER_IF = 4, SNN_LAYER_BOOSTED = 5,
       SNN_LAYER_CURRENT = 6, SNN_LAYER_IZH = 7, SNN_LAYER_SRM0 = 8, SNN_LAYER_CSRM = 9, SNN_LAYER_SIF = 10, SNN_LAYER_PASS = 11 };
/* SNN_LAYER_SIF (conversion/nodes.py:8, SubtractiveResetIFNodes; `summed` at the end of snn_layer_desc) and SNN_LAYER_PASS
 * (conversion/nodes.py:122, PassThroughNodes: `s` and `current` only -- inject_v and ext_current are SNN_ERR_UNSUPPORTED, and
 * every connection into it must be POOL, PERMUTE or PAD, whose outputs are 0 or 1), with SNN_CONN_PERMUTE / SNN_CONN_PAD
 * (conversion/topology.py: no `w`; the gat_* fields at the end of snn_conn_desc; propagation only, refused like POOL), were added
 * the same way: generic plan only, SNN_ABI_VERSION unchanged.  */
/* SNN_LAYER_SRM0 (nodes.py:1555; generic plan only, needs snn_run_desc.rng) with the srm_* fields at the end of snn_layer_desc, and
 * SNN_RULE_RMAX (learning.py:2858; a DENSE connection into an SRM0 layer, batch 1) with rmax_tc_c at the end of snn_conn_desc,
 * were added the same way: SNN_ABI_VERSION unchanged.  */
/* SNN_LAYER_CSRM (nodes.py:1319; generic plan only) with the csrm_* fields at the end of snn_layer_desc, and the win_* fields at
 * the end of snn_conn_desc -- a DENSE connection into a CSRM layer propagates its window: snn_prop_window_f32 --, were added the
 * same way: SNN_ABI_VERSION unchanged.  */
/* SNN_CONN_LOCAL (LocalConnection1D / 2D / 3D, rules NONE or POSTPRE, generic plan only) and the local_* fields at the end of
 * snn_conn_desc were added without changing SNN_ABI_VERSION: the change is purely additive.  A library built before it is
 * still refused at load, because the Python binding looks up every symbol declared here and such a library lacks
 * snn_prop_local_f32 / snn_local_postpre; tests/test_abi.py compares sizeof(snn_conn_desc) with the ctypes mirror.  */
/* SNN_CONN_CONVND (Conv1dConnection / Conv3dConnection, rules NONE or POSTPRE, generic plan only) and the conv_* fields
 * after them were added the same way, again without changing SNN_ABI_VERSION.  So were SNN_CONN_SPARSE (SparseConnection:
 * propagation only -- any rule, norm, mask or weight monitor is SNN_ERR_INVALID --, generic plan only) and the sparse_* fields.  */
/* SNN_CONN_POOL (MaxPool1d / 2d / 3dConnection: no `w`; firing_rates and the pool_* fields) and SNN_CONN_MEANFIELD
 * (MeanFieldConnection: `w` of w_numel elements) came the same way: propagation only -- a rule is SNN_ERR_UNSUPPORTED, a norm,
 * mask, bias or weight monitor SNN_ERR_INVALID --, generic plan only, SNN_ABI_VERSION unchanged.  */
/* SNN_CONN_AVGPOOL (AvgPool2dConnection, f18: no `w`, no state; the avgp_* fields in front of snn_conn_desc's last field) came the same way:
 * propagation only, refused like POOL, generic plan only, SNN_ABI_VERSION unchanged.  Its outputs are fractions, so it may not
 * feed a PASS layer.  */
enum { SNN_CONN_MCC = 0, SNN_CONN_DENSE = 1, SNN_CONN_CONV2D = 2, SNN_CONN_LOCAL = 3, SNN_CONN_CONVND = 4, SNN_CONN_SPARSE = 5,
       SNN_CONN_POOL = 6, SNN_CONN_MEANFIELD = 7, SNN_CONN_PERMUTE = 8, SNN_CONN_PAD = 9, SNN_CONN_AVGPOOL = 10 };
enum { SNN_RULE_NONE = 0, SNN_RULE_POSTPRE = 1, SNN_RULE_MSTDP = 2, SNN_RULE_HEBBIAN = 3, SNN_RULE_WDPOSTPRE = 4,
       SNN_RULE_MSTDPET = 5, SNN_RULE_RMAX = 6 };

typedef struct {
    int kind;                   /* SNN_LAYER_* */
    int n;                      /* neurons per sample */
    snn_dc_params p;            /* LIF uses p.lif only; INPUT uses p.lif.traces/trace_* only */
    float *v, *refrac, *x, *theta;   /* state [B,n] ([n] for theta); NULL where the layer has none */
    uint8_t *s;                 /* [B,n] spikes at entry, updated in place (INPUT: entry value, read only) */
    const uint8_t *ext_spikes;  /* INPUT: the [T,B,n] input tensor (aliased per step, never copied) */
    uint8_t *raster_s;          /* nullable [T,B,n] spike monitor */
    float *raster_v;            /* nullable [T,B,n] voltage monitor */
    float *current;             /* [B,n] scratch for the summed input current (non-INPUT layers) */
    /* run(..., clamp= / unclamp= / injects_v=), network.py:395-429 (nullable; handled by the generic plan):
     * after the layer's step  s[:, clamp] = 1, then s[:, unclamp] = 0  (u8 masks [n], or [T,n] when *_per_step);
     * before it               v += inject_v  (f32 [n] broadcast over the batch, or [T,...] when inject_per_step, each
     *                         slice [inject_len] with inject_len = n or B*n) */
    const uint8_t *clamp, *unclamp; int clamp_per_step, unclamp_per_step;
    const float *inject_v; int inject_per_step; int inject_len;
    /* run(inputs={<non-Input layer>: current}), network.py:386-392 (nullable; generic plan): f32 [T,B,n], slice t is added
     * to the layer's summed input current after the connections' contributions, before the layer steps */
    const float *ext_current;
    /* LIF layers with per-neuron thresholds (nodes.py:425-498: `thresh` given as a tensor): nullable f32 [n] that replaces
     * p.lif.thresh, broadcast over the batch; on any other kind it is read as pv.v[SNN_PV_THRESH] (see `pv` below).  Generic plan (a graph that has one is not offered to the fused plans).  (ABI 8) */
    const float *thresh_vec;
    /* CURRENT: aux = the synaptic current i [B,n], aux_decay = i_decay.  IZH: aux = the recovery variable u [B,n]; izh_a .. izh_d
     * f32 [n]; izh_St f32 [n,n], the lateral matrix transposed (snn_izh_step).  MCP has no refrac; BOOSTED / IF / CURRENT / IZH
     * use the p.lif fields their snn_*_step lists.  clamp / unclamp / inject_v / ext_current apply as for LIF. */
    float *aux; float aux_decay;
    const float *izh_a, *izh_b, *izh_c, *izh_d, *izh_St;
    /* Per-neuron parameters (f10): pv.v[SNN_PV_*] nullable f32 [n] vectors that take the place of the scalars in p / aux_decay.
     * A layer with any of them sends the graph to the generic plan, as thresh_vec does; a vector its kind does not read is
     * SNN_ERR_INVALID.  Added at the end without changing SNN_ABI_VERSION, like the fields above. */
    snn_pervec pv;
    /* SRM0: eps_0, rho_0, d_thresh and the layer's s_prob / rho [B,n] f32 outputs (snn_srm0_step).  The layer draws from
     * snn_run_desc.rng, within a timestep behind the Probability masks of the input gathering and in layer order. */
    float srm_eps0, srm_rho0, srm_dthresh;
    float *srm_sprob, *srm_rho;
    /* CSRM (snn_csrm_step): csrm_xwin the layer's window-current buffer f32 [B, csrm_wres, n] -- what its incoming connections'
     * snn_prop_window_f32 calls sum into, in place of `current` --, csrm_last its last_spikes f32 [B, csrm_wref, n] (oldest slot
     * first, updated in place), csrm_resk / csrm_refk the response and refractory kernels f32 [csrm_wres] / [csrm_wref]; theta [n]
     * and p (thresh, decay, lbound, traces, theta_decay, theta_plus, learning) as for DC.  ext_current is SNN_ERR_UNSUPPORTED. */
    float *csrm_xwin, *csrm_last;
    const float *csrm_resk, *csrm_refk;
    int csrm_wres, csrm_wref;
    /* SIF (snn_sif_step): the layer's `summed` f32 [B,n] -- Nodes(sum_input=True): every step adds the layer's raw input --, NULL
     * without sum_input.  Any other kind with it is SNN_ERR_INVALID.  Added like the fields above: SNN_ABI_VERSION stays. */
    float *summed;
    /* INPUT, real-valued (f17): ext_real != NULL makes the layer one.  ext_real is the f32 [T,B,n] input tensor (aliased per step),
     * s_real the f32 [B,n] values at entry (what connections read at t = 0), raster_real the nullable f32 [T,B,n] monitor copy; they
     * stand for ext_spikes / s / raster_s, which must then be NULL.  snn_net_run takes the generic plan; a connection out of such a
     * layer must be DENSE or CONV2D with rule NONE and a target that is no CSRM layer, else SNN_ERR_UNSUPPORTED.  On any other
     * kind the three are SNN_ERR_INVALID.  Added like the fields above: SNN_ABI_VERSION stays. */
    const float *ext_real;
    const float *s_real;
    float *raster_real;
} snn_layer_desc;

typedef struct {
    int kind;                   /* SNN_CONN_* */
    int src, dst;               /* indices into the layer array */
    float *w;                   /* [Nin,N] (CONV2D: [Cout,Cin,KH,KW]) */
    const float *bias;          /* nullable */
    int cin, h, wd, cout, kh, kw, stride, pad;   /* CONV2D geometry */
    int rule;                   /* SNN_RULE_* */
    float nu0, nu1;
    int use_dt;                 /* 1: MCC PostPre multiplies updates by dt */
    float wdecay;               /* multiplicative decay actually applied (1.0 = none) */
    int has_min; float wmin; int has_max; float wmax;
    float *p_plus, *p_minus;    /* MSTDP state [B,Nin] / [B,N] */
    uint8_t *s_src_prev, *s_tgt_prev;
    float reward; const float *reward_vec; float a_plus, a_minus, decay_plus, decay_minus;
    int has_norm; float norm; int norm_abs;   /* post-run normalisation (norm_abs: Connection) */
    /* Weight(norm_frequency="time step") (f16): non-zero -- the connection's Weight is normalised in EVERY timestep, right behind the
     * propagation that read its old values and before the step's learning update, learning or not, and the run's closing
     * normalisation skips the connection.  1: through snn_prop_cascade_f32 (a feature pipeline: snn_prop_mcc_pipe_f32) and
     * snn_normalize(_pv); 2: through snn_prop_cascade_norm_f32 / snn_prop_cascade_norm_pv_f32, one launch (pipe_n 0 only) -- the same bits.  Needs has_norm
     * (norm / norm_vec, norm_ws) with norm_abs 0 on an MCC connection with an f32 `w`: anything else with it is SNN_ERR_INVALID.  It
     * sends the graph to the generic plan.  The field takes what was padding in front of norm_ws: no offset and no size changes,
     * SNN_ABI_VERSION stays. */
    int norm_step;
    float *norm_ws;             /* [N] scratch when has_norm */
    float *e_trace;             /* MSTDPET: dense eligibility trace [Nin,N]; CONV2D + MSTDP: the eligibility [Cout,Cin*KH*KW]
                                   (p_plus is then [Cin,H,W], p_minus [Cout,OH*OW]; batch 1, s_*_prev unused) */
    float decay_e, tc_e;        /* MSTDPET: exp(-dt / tc_e_trace), tc_e_trace */
    float *rule_ws;             /* CONV2D + PostPre / Hebbian / WeightDependentPostPre: scratch of 2 * B * Cout*Cin*KH*KW floats */
    const uint8_t *mask;        /* nullable [Nin,N] (same layout as w): weights forced to zero after every step's update --
                                   run(..., masks=) / LocalConnection.mask, topology.py:129-133 (generic plan) */
    float *raster_w;            /* nullable [T, numel(w)] weight monitor (Monitor / NetworkMonitor on a connection's `w`,
                                   monitors.py:94-111,222-262): w as it stands at the END of every timestep, i.e. after that
                                   step's learning update and mask and before the post-run normalisation (generic plan) */
    /* LOCAL: w is [cin, local_F*local_conv_prod, local_kernel_prod]; local_src the int32 [cin, local_conv_prod,
     * local_kernel_prod] gather table of snn_prop_local_f32; local_n_src == the source layer's n.  has_norm: every
     * [local_kernel_prod] row scaled to sum `norm` (snn_normalize_conv2d, topology.py:1601 / :1748-1759 / :1898). */
    const int *local_src;
    int local_F, local_conv_prod, local_kernel_prod, local_n_src;
    /* CONVND: w is [cout, cin, conv_kd, kh, kw]; the source is [cin, conv_d, h, wd] (conv1d: conv_nd 1, conv_d = h = conv_kd
     * = kh = 1), stride / pad isotropic.  conv_pp_src: the int32 [conv_pp_rows, cin*conv_kd*kh*kw] PostPre gather table of
     * snn_convnd_postpre (conv_pp_rows == the target's positions); rule_ws its mask scratch.  has_norm is 0: the caller
     * normalises after the run, as for CONV2D. */
    int conv_nd, conv_d, conv_kd;
    const int *conv_pp_src;
    int conv_pp_rows;
    /* MCC with a feature pipeline (snn_prop_mcc_pipe_f32; generic plan only, no fused plan is offered such a graph).  pipe_n == 0:
     * the single Weight in `w`, as before.  pipe_n > 0: op k is (pipe_kind[k], pipe_val[k], pipe_scalar[k]); a MUL_DRAW op's
     * pipe_val is its f32 probabilities and pipe_bits[k] its uint32 [S, ceil(N/32)] workspace, filled by snn_mcc_bernoulli from
     * snn_run_desc.rng once per compute() of the reference, in pipeline order.  `w` is then the Weight the rule and the norm
     * refer to, NULL for a pipeline without one (rule NONE, has_norm 0).  Added like the fields above: SNN_ABI_VERSION stays. */
    int pipe_n;
    int pipe_kind[SNN_MCC_MAX_PIPE];
    const void *pipe_val[SNN_MCC_MAX_PIPE];
    int pipe_scalar[SNN_MCC_MAX_PIPE];
    uint32_t *pipe_bits[SNN_MCC_MAX_PIPE];
    /* SPARSE: the compiled form of snn_prop_sparse_f32 (ptr / col / val / nnz); `w` is NULL -- nothing learns, normalises, masks
     * or monitors a sparse matrix --, bias nullable.  Added like the fields above: SNN_ABI_VERSION stays. */
    const int *sparse_ptr;
    const uint8_t *sparse_col;
    const float *sparse_val;
    int sparse_nnz;
    /* POOL: the arguments of snn_prop_pool_f32 -- firing_rates f32 [B, pool_c, pool_in...] (the connection's state, updated every
     * timestep), three ints per geometry field (leading dimensions padded as there), pool_decay; `w` is NULL.  MEANFIELD: `w`
     * holds w_numel elements (snn_prop_meanfield_f32).  Added like the fields above: SNN_ABI_VERSION stays. */
    float *firing_rates;
    int pool_c, pool_in[3], pool_k[3], pool_stride[3], pool_pad[3], pool_dil[3];
    float pool_decay;
    int w_numel;
    /* RMAX (snn_rmax_step): e_trace is the rule's dense eligibility trace [Nin,N], tc_e its tc_e_trace, rmax_tc_c its tc_c; the
     * target's s_prob is read from the target layer's srm_sprob, the source's trace from its x. */
    float rmax_tc_c;
    /* A DENSE connection into a CSRM layer: `window` = 1, win_ring the connection's window of source spikes u8 [B, win_size, Nin]
     * kept as a ring, win_head the physical slot holding its OLDEST entry at the start of the run (the run leaves the oldest
     * entry in slot (win_head + T) mod win_size); win_size == the target's csrm_wres.  Any other kind into a CSRM layer, or
     * `window` on a connection into another layer kind, is SNN_ERR_INVALID. */
    int window;
    uint8_t *win_ring;
    int win_head, win_size;
    /* PERMUTE / PAD: the geometry of snn_prop_gather_f32 -- output extents, source extents in the output's dimension order, the
     * source stride and the leading offset per output dimension (three ints each, missing leading dimensions 1 / 1 / 0 / 0).
     * prod(gat_out) == the target's n; `w` is NULL.  Added like the fields above: SNN_ABI_VERSION stays. */
    int gat_out[3], gat_src[3], gat_stride[3], gat_off[3];
    /* The element type of `w` (SNN_W_*): 0 float32, as ever; 1 float16 / 2 bfloat16 -- `w` then points at 2-byte elements and the
     * connection runs snn_prop_cascade_h16 / snn_stdp_postpre_h16 / snn_normalize_h16.  MCC with one Weight only (pipe_n 0), rule
     * NONE or POSTPRE, no weight monitor, no mask: anything else is SNN_ERR_UNSUPPORTED.  A non-zero w_dtype sends the graph to the
     * generic plan, as per-neuron parameters do.  Added like the fields above: SNN_ABI_VERSION stays. */
    int w_dtype;
    /* Per-synapse learning rates / bounds and a per-target norm (f13 above): `syn` names the tensors among nu0, nu1, wmin, wmax
     * (the scalar fields above hold the others), norm_vec the device [target n] norms (has_norm 1; `norm` is then unused).  DENSE
     * and MCC connections with an f32 `w` and a rule of the dense family (POSTPRE, HEBBIAN, WDPOSTPRE, MSTDP, MSTDPET; norm_vec
     * also with NONE) only: anything else with one of these pointers is SNN_ERR_UNSUPPORTED.  Any of them sends the graph to the
     * generic plan, as per-neuron layer parameters do.  Added like the fields above: SNN_ABI_VERSION stays. */
    snn_synparams syn;
    const float *norm_vec;
    /* Time-averaged updates (f14 above): avg_k = the rule's average_update (0: none), avg_ring0 the ring f32 [avg_k, Nin, N] of
     * MSTDP / MSTDPET and PostPre's pre ring, avg_ring1 PostPre's post ring, avg_continuous its continues_update, avg_squeeze
     * reduction = torch.squeeze.  avg_i0 / avg_i1 are the ring indices at the START of the run -- per-call values like `reward`: timestep
     * t writes slot (avg_i + t) mod avg_k, and the caller advances its own index by T afterwards (a PostPre term whose rate is 0
     * never moves).  MCC connections with an f32 `w`, rules POSTPRE, MSTDP and MSTDPET, scalar rates and bounds (`syn` empty):
     * anything else with avg_k != 0 is SNN_ERR_UNSUPPORTED, avg_k > SNN_AVG_MAX_TERMS too; a missing ring or an index outside
     * [0, avg_k) is SNN_ERR_INVALID.  avg_k != 0 sends the graph to the generic plan.  Added like the fields above. */
    float *avg_ring0, *avg_ring1;
    int avg_k, avg_continuous, avg_squeeze, avg_i0, avg_i1;
    /* The rule's batch reduction (f15 above), SNN_REDUCE_*; 0 = SUM keeps every plan and kernel the connection had.  Another value
     * sends the graph to the generic plan, whose update calls take it through the *_red entry points (rules POSTPRE, HEBBIAN,
     * WDPOSTPRE and MSTDP; MSTDPET, RMAX, MSTDP on a CONV2D connection and NONE ignore it).  Outside the enum: SNN_ERR_INVALID.
     * Added like the fields above: SNN_ABI_VERSION stays. */
    int reduce;
    /* AVGPOOL: the arguments of snn_prop_avgpool2d_f32 -- avgp_c channels, two ints per geometry field, avgp_ceil its ceil_mode,
     * avgp_include_pad its count_include_pad, avgp_divisor its divisor_override (0: none); `w` is NULL.  avgp_c * the plane must
     * be the source's n and avgp_c * the pooled plane the target's, else SNN_ERR_INVALID.  Added without changing
     * SNN_ABI_VERSION, like the fields above; they stand in front of `activity`, which stays the descriptor's last field (the
     * library and its binding are built from this one header: tests/test_abi.py compares the sizes). */
    int avgp_c, avgp_in[2], avgp_k[2], avgp_stride[2], avgp_pad[2];
    int avgp_ceil, avgp_include_pad, avgp_divisor;
    /* MulticompartmentConnection(traces=True) (topology.py:415-435, :473-474): nullable f32 [B, target n], the connection's own
     * summed signal of the step.  With it the connection propagates into `activity` (accumulate = 0) and one elementwise launch
     * feeds the target: current = activity for the target's first connection, current = current + activity behind it -- the
     * arithmetic of the accumulate path's `*dst + acc`, so the currents keep their bits.  MCC only (any pipeline, any w_dtype):
     * another kind with it is SNN_ERR_INVALID.  It sends the graph to the generic plan.  To record it, name it in
     * snn_run_desc.records.  Added like the fields above: SNN_ABI_VERSION stays. */
    float *activity;
} snn_conn_desc;

/* What a connection needs to have its product's body chosen on the device (snn_prop_dense_auto_f32 above): one entry per
 * connection, in a table of its own beside the snn_conn_desc array (snn_net_run_props below) -- the descriptors keep their layout.
 * prop_flags: the connection's int32 [ceil(B / 16)] device scratch -- with it a DENSE connection fed by spike bytes (no window, not a
 * real-valued Input) CAN propagate through snn_prop_dense_auto_f32 on the generic plan; prop_counters: two device int32 words
 * {matrix tile-steps, event tile-steps} that the caller keeps across runs (nullable; they wrap after 2^31 - 1 tile-steps).
 * prop_auto != 0: the connection's owner ASKS for the device's choice.  Under the rule (snn_set_dense_prop_mode 0) a connection
 * takes snn_prop_dense_auto_f32 only if it is asked for and has at least 256 source neurons -- the choice costs a second launch
 * every step, 3 to 6 us however sparse the spikes are, so nobody pays it unasked; every other connection keeps the single launch
 * of snn_prop_dense_f32, as without the table.  Modes 1 and 2 (tests, measurements) take every connection that has prop_flags.
 * prop_auto without prop_flags is SNN_ERR_INVALID.  Ignored by every other kind and by the fused plans, which keep the event-driven form; an
 * MCC connection sums in ATen's cascade order, which a single chain cannot reproduce, and stays event-driven too. */
typedef struct {
    int prop_auto;
    int *prop_flags, *prop_counters;
} snn_conn_prop;

typedef struct {
    int B, T;
    float dt;
    int learning;               /* Network.learning */
    const float *noise_q;       /* pre-drawn Exp(1) stream for one_spike (see snn_dc_step); nullable */
    long long q_len;
    snn_rng_state *rng;         /* OR: device generator state (preferred; noise_q ignored when set) */
    float *qbuf;                /* with rng: scratch of B * max(DC layer n) floats */
    void *workspace;            /* device scratch for fused plans (snn_net_workspace_bytes); nullable */
    unsigned long long workspace_bytes;
    long long *cursor;          /* device int64[2] */
    int *status;                /* device int32[1]: 0, SNN_ERR_NOISE or SNN_ERR_TIMEOUT after the run */
    int one_step;               /* network.py:388-393 one_step=True: every layer's input is computed right before its own step
                                   from the CURRENT spikes of its sources (those already stepped in this timestep contribute
                                   their new spikes) -- a feed-forward pass per timestep.  Generic plan only. */
    int plan;                   /* 0 = automatic, 1 = generic per-operator launches, 2 = fused plans in their
                                   one-launch-per-timestep form (what a caller re-runs with after SNN_ERR_TIMEOUT),
                                   3 = automatic, but never the lean form of a plan (what a caller re-runs with after
                                   SNN_ERR_RETRY).  A run that reports either status has left every caller-owned STATE
                                   tensor untouched. */
    int *status2;               /* nullable device int32[1] (zeroed by the caller).  Pipelined callers -- those that do not read
                                   *status back before they enqueue the next run -- pass it to have the SECOND attempt of a lean
                                   plan enqueued right behind the first: the general form of the same plan, on the device gated
                                   on *status == SNN_ERR_RETRY (its workgroups return at once otherwise), reporting into *status2.
                                   Afterwards: the run succeeded iff *status == 0, or *status == SNN_ERR_RETRY and *status2 == 0.
                                   (ABI 8) */
    unsigned long long *host_state; /* nullable: 16 bytes of HOST memory that belong to `workspace` -- zeroed by the caller whenever the
                                   workspace is (re)allocated or written by anybody else, otherwise left alone.  The library notes there
                                   what it knows about the workspace's content, so that consecutive pipelined runs need not clear their
                                   exchange area with a memset each (the gated second attempt does it for the next run).  (ABI 8) */
    /* State monitors (snn_record_segments above): n_records segments, each a float32 tensor the generic plan's kernels update in
     * place (a layer's x, theta, refrac_count, i; a connection's activity) and its [T, ...] recording.  The run calls
     * snn_record_segments(records, n_records, t) at the END of timestep t -- behind the layers' steps, the clamps, the learning
     * updates, the masks and the weight-monitor copies, where the reference records (network.py:459-461); with one_step at the
     * same point.  n_records > 0 sends the graph to the generic plan, as a weight monitor does.  n_records < 0, a NULL table with
     * n_records > 0 or a segment snn_record_segments refuses: SNN_ERR_INVALID before anything runs.  Added at the end without
     * changing SNN_ABI_VERSION, like every additive field so far. */
    const snn_record_segment *records;
    int n_records;
} snn_run_desc;

/* Runs T timesteps.  Asynchronous; the caller synchronises the stream before reading *status /
 * cursor[0].  Picks a fused plan when the graph matches one (snn_plan_name reports which).  */
int snn_net_run(const snn_layer_desc *h_layers, int n_layers, const snn_conn_desc *h_conns, int n_conns,
                const snn_run_desc *h_run, snn_stream_t stream);
/* snn_net_run with a snn_conn_prop per connection (h_props [n_conns], host memory; NULL: exactly snn_net_run).  The table is read
 * by the generic plan only; every other argument, result and plan is snn_net_run's.  (ABI 8, additive) */
int snn_net_run_props(const snn_layer_desc *h_layers, int n_layers, const snn_conn_desc *h_conns, int n_conns,
                      const snn_conn_prop *h_props, const snn_run_desc *h_run, snn_stream_t stream);
/* Device scratch (bytes) a fused plan would need for this network; 0 if none applies.  A run
 * whose descriptor carries less falls back to the generic plan.                               */
unsigned long long snn_net_workspace_bytes(const snn_layer_desc *h_layers, int n_layers, const snn_conn_desc *h_conns,
                                           int n_conns, const snn_run_desc *h_run);
/* Name of the plan the last snn_net_run on this thread used ("generic", "dc2015-fused", ...). */
const char *snn_plan_name(void);
/* Which resident form of the DiehlAndCook2015 plan the last such run of this process took: 0 = general form, 1 / 2 / 3 = first /
 * second / third generation of the lean form (csrc/snn_dc2015_resident.hip, snn_dc2015_async.hip), -1 = one launch per timestep or no
 * such run yet.  ABI 7; a diagnostic for bench.py and the tests (the plan NAME stays "dc2015-resident-lean" for all lean forms). */
int snn_dc2015_last_form(void);
/* Profiling aid (bench.py roofline): when stride > 0, snn_net_run brackets the launches of every
 * stride-th timestep with hipEvents recorded on the run's stream (at most 64 samples per run).
 * snn_profile_collect (call after synchronising the stream) returns the summed elapsed
 * milliseconds and the sample count, and clears the samples.                                 */
void snn_profile_enable(int stride);
int snn_profile_collect(double *h_sum_ms, int *h_samples);
/* Fused-plan bookkeeping: runs of the dc2015 plans issued as plain launches.  The hipGraph capture-and-replay path these
 * counters were made for has been removed: *h_captured and *h_replayed are always 0 (kept: the ABI is additive-only). */
void snn_graph_stats(int *h_plain, int *h_captured, int *h_replayed);
/* Force a plan for testing: 0 = automatic, 1 = generic per-operator launches only,
 * 2 = fused plans in their one-launch-per-timestep form (no resident kernel), 3 = no lean forms. */
void snn_set_plan_mode(int mode);

/* ---- (e) multi-GPU: one process per GPU, RCCL over xGMI ----------------------------------------
 * SURVEY.md 8(e).  Rank 0 calls snn_dist_unique_id and distributes the 128 bytes; every rank then calls snn_dist_init
 * with the HIP device it will use already current.  snn_dist_allreduce_dw = the north-star schedule (sum the
 * per-input weight / threshold deltas over ranks, in place); snn_dist_allgather_step = the exact per-timestep mode
 * (every rank's packed step factors, concatenated in rank order).  Both are stream-ordered and asynchronous.
 * SNN_ERR_UNSUPPORTED: no RCCL library could be opened on this machine.                               */
typedef struct snn_dist snn_dist;
int snn_dist_unique_id(void *h_id128);
int snn_dist_init(int rank, int world, const void *h_id128, snn_dist **h_out);
int snn_dist_world(const snn_dist *d, int *h_rank, int *h_world);
int snn_dist_allreduce_dw(snn_dist *d, float *buf, long long count, snn_stream_t stream);
int snn_dist_allgather_step(snn_dist *d, const void *send, void *recv, long long bytes_per_rank, snn_stream_t stream);
int snn_dist_destroy(snn_dist *d);

#ifdef __cplusplus
}
#endif
#endif /* SNNHIP_H */
