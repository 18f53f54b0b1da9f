/* rfn_hip.h — C ABI of librfn_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the RFN hot path.
 *
 * The reference (cdglissov/recurrent-flows-msc) has no FFI: its boundary for this path is the Python class API of
 * `Flow/glow_modules.py`, `Flow/glow.py` and `Utils/modules.py` (ConvLSTM).  Each entry point below replaces the
 * torch-op sequence of the cited reference lines; the Python host side (recurrent-flows-msc_amd/{Flow,Utils,RFN})
 * keeps the reference's class names, signatures and state_dict keys and calls these through ctypes
 * (recurrent-flows-msc_amd/rfn_hip/lib.py).  See INTEGRATION.md for the binding a maintainer would add.
 *
 * Conventions
 *   - every tensor is fp32, NCHW, device memory, 4-byte aligned; "ns" arguments are the frame (dim-0) stride in
 *     ELEMENTS, so a channel-slice view of a bigger tensor can be passed without a copy; the channel stride is H*W;
 *   - N is the number of frames in the launch (the host time-batches B*(T-1) frames), HW = H*W;
 *   - all functions enqueue on `stream` (a hipStream_t passed as void*) and never synchronise; the only allocation the
 *     library makes is ONE grow-only scratch buffer per device for the split-K convolutions (few-pixel shapes: the K
 *     slices write partial outputs there and a second kernel adds them in a fixed order -- no float atomics, results are
 *     bit-reproducible).  It grows on first use of a larger shape (hipMalloc; refused with an error while the stream is
 *     being captured into a hipGraph: run the shape eagerly once first) and serves every stream of the device, so
 *     split-K convolutions on DIFFERENT streams of one device must not overlap in time;
 *   - return value: 0 on success, otherwise a hipError_t / negative argument-check code; rfn_last_error() gives text;
 *   - global state: the (thread-local) last-error string, and four developer knobs that the kernel selectors read ONCE
 *     from the environment at their first call and then keep for the life of the process: RFN_CONV_WS (0: no
 *     weight-stationary kernels), RFN_WGRAD_DMA (0: no LDS-DMA ring kernels), RFN_CONV_VARIANT, RFN_WGRAD_BPX128
 *     (tile / split-K experiments; unset = production choice).
 *     They pick between
 *     kernels that compute the same result; nothing else is cached between calls, and the library is safe to call from
 *     several host threads on distinct streams.  The *_kernel_label_* queries answer with the same knobs applied, so a
 *     caller may cache their answers for the life of the process.
 */
#ifndef RFN_HIP_H
#define RFN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rfn_stream_t;

/* Version of this ABI, checked by the loader.  2: the conv weight pack from a DEVICE descriptor table is removed (host
 * descriptors only: rfn_pack_conv_weights_hostdescs_bf16x3); rfn_coupling_po_fwd gained the mask outputs m1 / m2,
 * rfn_stepbn_bwd_f32 its stage / world arguments; the log-det argument of rfn_glow_shell_fwd_f32 is a written
 * [blocks][slots] partials buffer (rfn_logdet_reduce_f32) and that of rfn_invconv_weights_fwd_f32 is written, not
 * accumulated. */
int rfn_abi_version(void);
const char* rfn_last_error(void);

/* ---- a1  Squeeze2d.forward  (Flow/glow_modules.py:298-310): out[b,4c+2i+j,h,w] = in[b,c,2h+i,2w+j]; undo = inverse.
 * C,H,W are the INPUT dims.  x_ns / y_ns: frame strides of input / output. Bit-exact copy. */
int rfn_squeeze2d_f32(const float* x, long x_ns, float* y, long y_ns, int N, int C, int H, int W, int undo,
                      rfn_stream_t stream);

/* ---- a3  ActNorm.initialize  (glow_modules.py:22-31): per-channel mean and UNBIASED variance over (N,H,W).
 * mean[C], var[C] are overwritten. */
int rfn_channel_stats_f32(const float* x, long x_ns, float* mean, float* var_unbiased, int N, int C, int HW,
                          rfn_stream_t stream);

/* ---- a3+a4  ActNorm.forward + InvConv.forward fused  (glow_modules.py:38-45, 209-216):
 *   y = (x + bias[c]) * exp(logs[c]);  z[n,:,p] = Wm · y[n,:,p]      (Wm is the C×C matrix built on the host from
 *   P,L,U,log_s, glow_modules.py:188-205).  The log-det terms (Σlogs + Σlog_s)·HW are parameter-only and are added
 *   by the host. */
int rfn_actnorm_invconv_fwd_f32(const float* x, long x_ns, const float* bias, const float* logs, const float* Wm,
                                float* z, long z_ns, int N, int C, int HW, rfn_stream_t stream);
/* backward of the above: given gz, recomputes y; gx = exp(logs)·Wmᵀgz; gW += Σ gz yᵀ; gbias += Σ gy·exp(logs);
 * glogs += Σ gy·y.  gW[C*C], gbias[C], glogs[C] are ACCUMULATED into (caller zeroes them). */
int rfn_actnorm_invconv_bwd_f32(const float* x, long x_ns, const float* bias, const float* logs, const float* Wm,
                                const float* gz, long gz_ns, float* gx, long gx_ns, float* gW, float* gbias,
                                float* glogs, int N, int C, int HW, rfn_stream_t stream);
/* ---- a4  InvConv.get_weight for the K steps of a flow level  (glow_modules.py:178-207, forward direction):
 *   W[k] = P[k] (lower[k] o tril(-1) + I)(upper[k] o triu(+1) + diag(sign_s[k] * exp(log_s[k]))),  W is [K][C][C];
 *   *logdet  = H*W * sum_k sum(log_s[k])   (written; the K steps are added in order by one workgroup: no atomics).
 * The five parameter arguments are HOST arrays of K device pointers (one per step: no stacking copies); K <=
 * RFN_INVCONV_MAX_STEPS, C <= RFN_INVCONV_MAX_CHANNELS (three C x C matrices in LDS).  Backward: from gW [K][C][C] and gc (gradient of the scalar, may be NULL) to
 * g_lower, g_upper [K][C][C] (zero outside their triangles) and g_log_s [K][C]. */
#define RFN_INVCONV_MAX_STEPS 32
#define RFN_INVCONV_MAX_CHANNELS 96
int rfn_invconv_weights_fwd_f32(const float* const* p, const float* const* lower, const float* const* upper,
                                const float* const* log_s, const float* const* sign_s, float* W, float* logdet, int K,
                                int C, int HW, rfn_stream_t stream);
int rfn_invconv_weights_bwd_f32(const float* const* p, const float* const* lower, const float* const* upper,
                                const float* const* log_s, const float* const* sign_s, const float* gW, const float* gc,
                                float* g_lower, float* g_upper, float* g_log_s, int K, int C, int HW, rfn_stream_t stream);
/* reverse direction (glow_modules.py:47-52, 217-221):  x = (Winv · z) * exp(-logs) - bias. */
int rfn_invconv_actnorm_rev_f32(const float* z, long z_ns, const float* bias, const float* logs, const float* Winv,
                                float* x, long x_ns, int N, int C, int HW, rfn_stream_t stream);

/* ---- a5.1/a5.2  Conv2dNorm / Conv2dZeros / ConvLSTM conv  (glow_modules.py:106-147, Utils/modules.py:335-340,368):
 * implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), stride 1, "same" padding, ks ∈ {1,3}.
 * Input channels [0,C1) are read from in1, [C1,C1+C2) from in2 (the torch.cat of glow_modules.py:273,355 and
 * Utils/modules.py:367 is never materialised); in2 may be NULL when C2 == 0.
 * wpk: weights packed by rfn_pack_conv_weight_f32.
 * Output channels [0,cout_split) go to out1, [cout_split,Cout) to out2 (out2 may be NULL when cout_split == Cout);
 * acc1/acc2 != 0 accumulates (out += result) instead of overwriting.
 * Epilogue (ep_mode), applied per output channel c before the store:
 *   0: y = a                                   (plain; used for dgrad)
 *   1: y = act((a + p0[c]) * exp(p1[c]))       (Conv2dNorm = conv + ActNorm, then ActFun; act 0 none,1 relu,2 leaky .2)
 *   2: y = (a + p0[c]) * exp(3*p1[c])          (Conv2dZeros)
 *   3: y = a + p0[c]                           (conv with bias; ConvLSTM)
 */
int rfn_conv2d_fwd_f32(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                       const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                       int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                       const float* p0, const float* p1, int act, rfn_stream_t stream);
/* Host-only label queries (here and below, *_kernel_label_*): the template instantiation the entry point named in the
 * comment launches for these arguments, e.g. "conv_mfma_kernel<1,2,2,2,2,32>", as a pointer to static storage.  Each is
 * answered by the very function the launcher switches on, needs no device, launches nothing, and takes every argument
 * the choice depends on.  This one: rfn_conv2d_fwd_f32. */
const char* rfn_conv2d_kernel_label_f32(int ks, int Cout, int N, int H, int W);

/* ---- split-precision variant of the same convolution ("bf16x3"): every fp32 operand x is split on the fly into two
 * bf16 numbers hi + lo and a*b is formed as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi by three v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation (relative error of a product <= 2^-16; measured nll error ~1e-5 relative, budget 1e-4).  Inputs,
 * outputs, epilogues and argument meaning are identical to rfn_conv2d_fwd_f32; wpk must come from
 * rfn_pack_conv_weight_bf16x3 (which also performs the hi/lo split of the weights). */
int rfn_conv2d_fwd_bf16x3(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                          const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                          int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                          const float* p0, const float* p1, int act, rfn_stream_t stream);
long rfn_packed_weight_size_bf16x3(int Cout, int Cin, int ks); /* in floats (4-byte units) */
int rfn_pack_conv_weight_bf16x3(const float* w, float* wpk, int Cout, int Cin, int ks, int transpose_flip,
                                rfn_stream_t stream);
/* "bf16x6": three bf16 pieces per operand (24 significant bits), six MFMAs per product -- fp32-grade results at twice
 * the cost of bf16x3 and a third of the fp32-MFMA kernel's; the forward convolutions of the flow levels the fused kernel
 * does not take ('mixed' arithmetic).  Same arguments as the bf16x3 functions; generic tile kernel only. */
long rfn_packed_weight_size_bf16x6(int Cout, int Cin, int ks);
int rfn_pack_conv_weight_bf16x6(const float* w, float* wpk, int Cout, int Cin, int ks, int transpose_flip,
                                rfn_stream_t stream);
int rfn_conv2d_fwd_bf16x6(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                          const float* wpk, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                          int cout_split, int acc1, int acc2, int N, int H, int W, int ks, int ep_mode,
                          const float* p0, const float* p1, int act, rfn_stream_t stream);
/* label query for rfn_conv2d_fwd_bf16x3 (npl = 2), rfn_conv2d_fwd_bf16x6 (npl = 3) and, with ep_mode = 4, cout_split =
 * Cout, C2 = 0 and acc1 = 0, rfn_conv2d_dgrad_act_bf16x3 (C1 = its Cin) */
const char* rfn_conv2d_kernel_label_bf16x3(int npl, int ks, int C1, int C2, int Cout, int cout_split, int acc1,
                                          int ep_mode, int N, int H, int W);

/* 3x3 / pad 1 convolution of an image with 1 .. 4 channels into 16 or 32 feature maps as plain fp32 FMAs (exact), one
 * thread per pixel: the first convolution of the frame extractor (Utils/modules.py:81, VGG_downscaler's 3x3 / stride 1 /
 * bias-free convolution applied to the input frames, called from RFN/RFN_new.py:127;
 * w is the torch weight [Cout][Cin][3][3], no epilogue), and its weight gradient for one input channel and 16 outputs
 * (gw [16][1][3][3], accumulated with float atomics: the caller zeroes it). */
int rfn_conv3x3_fewcin_supported(int Cin, int Cout);
int rfn_conv3x3_fewcin_fwd_f32(const float* in, long in_ns, int Cin, const float* w, float* out, long out_ns, int Cout,
                               int N, int H, int W, rfn_stream_t stream);
int rfn_conv3x3_c1_wgrad16_f32(const float* in, long in_ns, const float* g, long g_ns, float* gw, int N, int H, int W,
                               rfn_stream_t stream);

/* Data-gradient convolution fused with the backward of the PRODUCER conv's Conv2dNorm epilogue (ActNorm + ActFun,
 * glow_modules.py:139-142 + Utils/modules.py:8-19): with y = act((u+b)*exp(logs)) saved from the forward pass,
 *   g  = conv(gin, wpk)                    (wpk packed with transpose_flip = 1 / mode 1)
 *   out = g * act'(y) * exp(logs[c])       (= grad wrt u, what the producer's weight- and data-gradient consume)
 *   part[0][c] += Σ out  (= grad b),  part[1][c] += Σ g*y  (= grad logs)   over all frames and pixels
 * part is [2][Cout], accumulated with float atomics (one per workgroup / wave and channel): the caller zeroes it.
 * Cout % 64 == 0.  (rfn_conv2d_dgrad_act_rows_bf16x3: number of partial sums per channel the launch adds; informative.) */
int rfn_conv2d_dgrad_act_rows_bf16x3(int N, int H, int W, int ks, int Cout, int Cin);
int rfn_conv2d_dgrad_act_bf16x3(const float* gin, long gin_ns, int Cin, const float* wpk, const float* y, long y_ns,
                                const float* logs, int act, float* out, long out_ns, float* part, int Cout, int N,
                                int H, int W, int ks, rfn_stream_t stream);

/* Pack many weights at once: n descriptors in HOST memory, 64 per launch (the table travels in the kernel arguments).
 * The host collects the packs a step asks for back to back and hands them over in one call; rfn_pack_conv_weight_bf16x3
 * / _bf16x6 are the one-descriptor form of this call.  mode 0 forward, 1 data-gradient (transposed, taps mirrored),
 * 2 tap-expanded 1x1 form of a 3x3 conv with tiny Cout (w'[tap*Cout+co][ci] = w[co][ci][tap]); mode + 4: three planes
 * (bf16x6) instead of two.  Each wpk must hold rfn_packed_weight_size_bf16x3 (or _bf16x6) floats of the LOGICAL conv
 * (mode 2: Cout' = 9*Cout, ks' = 1). */
typedef struct {
    const float* w;
    float* wpk;
    int Cout, Cin, ks, mode;
} rfn_pack_desc;
int rfn_pack_conv_weights_hostdescs_bf16x3(const void* descs_host, int n, rfn_stream_t stream);

/* ---- a5 fused  AffineCoupling.net forward for the shallow levels (Flow/glow_modules.py:232-238 with :119-121 and
 * :139-142), csrc/coupling_po.hip: conv3x3 -> ActNorm -> act -> conv1x1 -> ActNorm -> act -> tap-expanded conv3x3 in
 * ONE kernel; the 256-channel hidden activations pass from layer to layer in registers (they are still written once:
 * the backward pass needs them).  Arithmetic "f16x3s": every operand is scaled by a power of two (per tensor for
 * weights, per block for the staged input, per pixel for the hidden activations) and split into two fp16 pieces
 * (22 significant bits); a product is three v_mfma_f32_32x32x16_f16 with fp32 accumulation, the scale undone in fp32.
 *   rfn_coupling_po_supported  1 when (N, C, Cc, Hd, H, W) is a shape the kernel takes (else use the unfused kernels):
 *       Hd = 256, square power-of-two maps, N*H*W a multiple of 128 (a workgroup round is 128 consecutive pixels of the
 *       (frame, pixel) sequence: rows of one frame, or two whole 8x8 frames) and one of the instantiated channel-group
 *       counts (NG = ceil((C/2 + Cc) / 8), NP = ceil(9C / 32), W): (3, 2, 32) and (5, 3, 16) = levels 0 / 1 of the
 *       canonical flow, (9, 5, 8) = its level 2, (9, 4, 32) = a C = 12 flow with 59..66 condition channels;
 *   rfn_coupling_po_packed_bytes / rfn_coupling_po_pack  the fragment-ordered weight stream of one coupling net
 *       (descs_device: device array of n rfn_po_pack_desc; one launch packs every net of a flow);
 *   rfn_coupling_po_fwd  z: output of ActNorm+InvConv [N, >=C/2, H, W] (channels [0, C/2) are read), cond [N, Cc, H, W];
 *       n1b/n1l, n2b/n2l: ActNorm bias / logs [256] of the hidden layers; act 0 none, 1 relu, 2 leaky .2.
 *       Outputs h1, h2 [N, 256, H, W] and P [N, 9C, H, W], P[tap*C + co] = sum_c w3[co][c][tap] h2[c]
 *       (rfn_tap_gather_f32 turns P into the Conv2dZeros output); m1 / m2 (nullable, rfn_coupling_po_mask_floats(N, H, W)
 *       floats each, 16-byte aligned): 1-bit masks "h <= 0" of h1 / h2 in the backward kernel's (round, thread,
 *       register) order -- act'(.) for rfn_coupling_po_bwd, 1/32 of the activations' bytes.
 * Backward of the same three convolutions' DATA path (backward of glow_modules.py:232-238), one kernel:
 *   rfn_coupling_po_bwd_supported / rfn_coupling_po_bwd_packed_bytes / rfn_coupling_po_pack_bwd  as above for the
 *       backward stream (w3 transposed + mirrored, w2 transposed; descs: w2, w3, dst, C are read); gradient images of
 *       C <= 8 channels on 32x32 / 16x16 maps and of 9..16 channels on 8x8 / 32x32 maps;
 *   rfn_coupling_po_bwd  go [N, C, H, W] = gradient at conv3's output ->
 *       ga2 = (conv3^T go) act'(h2) exp(n2l), ga1 = (w2^T ga2) act'(h1) exp(n1l)  [N, 256, H, W] each (the gradients at
 *       the outputs of conv2 / conv1: operands of the weight gradients and of conv1's data gradient), and
 *       part (rfn_coupling_po_bwd_part_floats(N, H, W) floats, written): per-workgroup sums over pixels of ga2 | ga1;
 *   rfn_coupling_po_bwd_finish  for n <= 16 nets (host arrays of n device pointers): ActNorm gradients
 *       out[i] = [gn1b | gn1l | gn2b | gn2l] (4 x 256) with gnb = sum of the part rows (nblk of them) and
 *       gnl[c] = sum_k w[c][k] gw[c][k] + nb[c] gnb[c]  (K1 = Cin * 9 elements per row of w1 / gw1, 256 of w2 / gw2). */
typedef struct {
    const float* w1;  /* [256][C/2 + Cc][3][3] */
    const float* w2;  /* [256][256][1][1] */
    const float* w3;  /* [C][256][3][3] */
    float* dst;       /* rfn_coupling_po_packed_bytes(Cin, C) bytes, 16-byte aligned */
    int Cin, C;
} rfn_po_pack_desc;
int rfn_coupling_po_supported(int N, int C, int Cc, int Hd, int H, int W);
long rfn_coupling_po_packed_bytes(int Cin, int C);
int rfn_coupling_po_pack(const void* descs_device, int n, rfn_stream_t stream);
int rfn_coupling_po_fwd(const float* z, long z_ns, const float* cond, long cond_ns, const void* wpk, const float* n1b,
                        const float* n1l, const float* n2b, const float* n2l, float* h1, long h1_ns, float* h2,
                        long h2_ns, float* P, long P_ns, float* m1, float* m2, int N, int C, int Cc, int H, int W, int act,
                        rfn_stream_t stream);
long rfn_coupling_po_mask_floats(int N, int H, int W);
/* Host-only queries of the weight streams' layout (the streams stay opaque to callers: sizes come from the
 * *_packed_bytes functions).  Change note: the first product's K order is dense -- units of 8 K-values, two per k-step;
 * full units are (tap, 8-channel group) over the 9 real taps, and where the leftover Cin % 8 channels have a narrow
 * instantiation (forward Cin 17..18 and 35..36, backward C = 4) they are the FIRST channels and form units of 8/r' taps
 * x r' channels -- instead of 5 tap pairs x ceil(Cin / 8) groups; streams of an older build are not interchangeable.
 *   rfn_coupling_po_k_order  unit < 0: the number of units of the forward (bwd = 0, Cin = C/2 + Cc) or backward
 *       (bwd = 1, Cin = C) stream; else the real taps [*tap0, *tap0 + *n_taps) and channels [*ch0, *ch0 + *n_ch) of
 *       that unit, and its k-step (unit / 2) as the return value; negative on a bad argument;
 *   rfn_coupling_po_ring_group  idx < 0: the number of LDS-ring groups of a round; else first fragment (1 KB each,
 *       fragment 0 = header) and fragment count of group idx in consumption order (C is not read with bwd = 1);
 *       (out-parameters are long long, the one integer pointee the loader's binding check knows);
 *   rfn_coupling_po_lds_bytes  dynamic LDS of the kernel instantiation that serves the shape (limit: 160 KB). */
int rfn_coupling_po_k_order(int Cin, int bwd, int unit, long long* tap0, long long* n_taps, long long* ch0,
                            long long* n_ch);
int rfn_coupling_po_ring_group(int Cin, int C, int bwd, int idx, long long* first_frag, long long* n_frags);
long rfn_coupling_po_lds_bytes(int Cin, int C, int W, int bwd);
int rfn_coupling_po_bwd_supported(int N, int C, int H, int W);
long rfn_coupling_po_bwd_packed_bytes(int C);
int rfn_coupling_po_pack_bwd(const void* descs_device, int n, rfn_stream_t stream);
long rfn_coupling_po_bwd_part_floats(int N, int H, int W);
int rfn_coupling_po_bwd(const float* go, long go_ns, const void* wpk, const float* n1l, const float* n2l,
                        const float* m_h1, const float* m_h2, float* ga2, long ga2_ns, float* ga1, long ga1_ns,
                        float* part, int N, int C, int H, int W, int act, rfn_stream_t stream);
int rfn_coupling_po_bwd_finish(const float* const* part, const float* const* w1, const float* const* gw1,
                               const float* const* n1b, const float* const* w2, const float* const* gw2,
                               const float* const* n2b, float* const* out, int n, int nblk, int K1,
                               rfn_stream_t stream);

/* ---- a5/a6 fused shell tail of GlowStep.forward (Flow/glow_modules.py:119-121 + :276-285): with P (tap-expanded
 * Conv2dZeros output, [N,9C,H,W]) the 3x3 shift-and-add, bias and exp(3 logs) scale are applied here and the result is
 * also written to o_out [N,C,H,W]; without P, o_in holds that result.  z [N,C,H,W] (frame stride z_ns): channels
 * [C/2, C) <- (z2 + o[0::2]) * exp(clamp(o[1::2])); logdet[n] = sum of the clamped log-scales is WRITTEN. */
int rfn_gather_affine_f32(const float* P, const float* o_in, long o_ns, const float* b3, const float* l3, float* o_out,
                          float* z, long z_ns, const float* scale, const float* scale_shift, float* logdet,
                          int clamp_type, int N, int C, int H, int W, rfn_stream_t stream);
/* backward of the affine coupling and of the Conv2dZeros epilogue in one launch: from gout (grad of the step's output)
 * and glogdet [N] (may be NULL) to gz (whole tensor: first half copied from gout, second half the coupling gradient) and
 * gpre = grad at the convolution output (what the weight / data gradient of conv3 consume).  gscale, gscale_shift [C/2]
 * (realnvp clamp only), gb3, gl3 [C] are ACCUMULATED into (caller zeroes them). */
int rfn_affine_zeros_bwd_f32(const float* zout, long zout_ns, const float* o, long o_ns, const float* gout, long gout_ns,
                             const float* glogdet, const float* scale, const float* scale_shift, const float* l3,
                             float* gz, long gz_ns, float* gpre, long gpre_ns, float* gscale, float* gscale_shift,
                             float* gb3, float* gl3, int clamp_type, int N, int C, int HW, rfn_stream_t stream);

/* ---- a6 shell BETWEEN two consecutive Glow steps of a level, one launch each way (Flow/glow.py:31-36 unrolled over
 * the K steps of a level).  Forward: the coupling tail of step k (as rfn_gather_affine_f32) then, when Wm != NULL, the
 * ActNorm + InvConv head of step k+1: znext = Wm ((z' + bias) * exp(logs)).  With P == o_in == NULL only the head runs
 * (first step of a level; z is then read only).
 * Log-det WITHOUT float atomics (a forward pass is bit-reproducible): `logdet` is this launch's buffer of per-workgroup
 * partial sums (rfn_glow_shell_fwd_ld_floats(N, C, H, W) floats, WRITTEN); rfn_logdet_reduce_f32 adds the partials of
 * n_launch consecutive such buffers per frame in a fixed order into logdet [N] (accumulate = 1: added to it). */
int rfn_glow_shell_fwd_f32(float* z, long z_ns, const float* P, const float* o_in, long o_ns, const float* b3,
                           const float* l3, float* o_out, const float* scale, const float* scale_shift, float* logdet,
                           int clamp_type, const float* bias, const float* logs, const float* Wm, float* znext,
                           long znext_ns, int ld_const, int N, int C, int H, int W, rfn_stream_t stream);
long rfn_glow_shell_fwd_ld_floats(int N, int C, int H, int W);
int rfn_logdet_reduce_f32(const float* part, int n_launch, float* logdet, int accumulate, int N, int C, int H, int W,
                          rfn_stream_t stream);
/* Host-only label queries of the shell launches (the structs the launchers themselves read; "unsupported" where the
 * launcher refuses).  Forward: "glow_shell_fwd_kernel PB=.. blocks=.. slots=.. lds=<bytes> ld=<frame | pow2x<G> | generic |
 * frame+generic> prod=<none | global | lds2 | lds4>" -- the log-det branch of the launch's blocks and the form of the
 * head's C x C product.  Backward (tail = 1: rfn_glow_shell_bwd_f32, 0: rfn_actnorm_invconv_bwd[_ld]_f32):
 * "actnorm_invconv_bwd_small_kernel<C,tail> grid=.. sweeps=.. lds=.." or "actnorm_invconv_bwd_kernel<tail> PB=.. grid=..
 * ny=.. gW=<split | owned> sweeps=.. lds=..".  rfn_glow_shell_supported: 1 when the forward head AND both backward entry
 * points accept the shape (C even; at most 144 channels), which is what a flow level needs. */
const char* rfn_glow_shell_fwd_kernel_label(int N, int C, int H, int W, int head);
const char* rfn_glow_shell_bwd_kernel_label(int N, int C, int HW, int tail);
int rfn_glow_shell_supported(int N, int C, int H, int W);
/* (ld_const = 1: the head also adds its ActNorm's parameter-only log-det term H*W * sum_c logs[c] to logdet[n],
 * glow_modules.py:47-52; the backward kernels below then add H*W * sum_n glogdet[n] to glogs.) */
/* Backward: rfn_actnorm_invconv_bwd_f32 of step k+1 (x = its input = step k's output, gz = gradient wrt its
 * post-InvConv tensor; gW, gbias, glogs accumulated) whose result feeds rfn_affine_zeros_bwd_f32 of step k from
 * registers (o .. gl3 are step k's, same meaning as there). */
int rfn_glow_shell_bwd_f32(const float* x, long x_ns, const float* bias, const float* logs, const float* Wm,
                           const float* gz, long gz_ns, float* gW, float* gbias, float* glogs, const float* o, long o_ns,
                           const float* glogdet, const float* scale, const float* scale_shift, const float* l3,
                           float* gz_prev, long gz_prev_ns, float* gpre, long gpre_ns, float* gscale,
                           float* gscale_shift, float* gb3, float* gl3, int clamp_type, int ld_const, int N, int C,
                           int HW, rfn_stream_t stream);
int rfn_actnorm_invconv_bwd_ld_f32(const float* x, long x_ns, const float* bias, const float* logs, const float* Wm,
                                   const float* gz, long gz_ns, float* gx, long gx_ns, float* gW, float* gbias,
                                   float* glogs, const float* glogdet, int N, int C, int HW, rfn_stream_t stream);

/* ---- 3x3 convolution (stride 1, pad 1) with few output channels (at most 64 on 32x32 and 16x16 maps, at most 96 on
 * 8x8 maps) and Cin % 32 == 0 input channels, bf16x3 arithmetic, one input tensor whose N * Cin * H * W * 4 bytes stay
 * below 0xFFFFFF00: the data gradient of the first coupling-net convolution at the three finest flow levels
 * (256 -> C/2 + Cc channels; backward of Flow/glow_modules.py:232-238).  rfn_dgrad_small_supported tells.  wpk: the
 * rfn_pack_conv_weight_bf16x3 buffer of the logical weight (transpose_flip = 1 of the forward weight for a data
 * gradient).  Output channels [0, cout_split) go to out1, the rest to out2; acc1 / acc2: add into what is there. */
int rfn_dgrad_small_supported(int N, int Cin, int Cout, int H, int W);
int rfn_conv3x3_smallcout_bf16x3(const float* in, long in_ns, int Cin, const float* wpk, float* out1, long out1_ns,
                                 float* out2, long out2_ns, int Cout, int cout_split, int acc1, int acc2, int N, int H,
                                 int W, rfn_stream_t stream);

/* Split-precision weight-gradient GEMM: gw[M][Nc] += Σ_{f,p} a[f][m][p] * b[f][n][p]  (a: [F,M,HW] frame stride a_ns,
 * b: [F,Nc,HW] frame stride b_ns; HW % 4 == 0, 16-byte aligned bases).  gw is accumulated with float atomics (caller
 * zeroes it).  1x1 weight gradients use it directly (a = output grad, b = conv input); 3x3 ones first expand the
 * smaller operand: b = rfn_im2col3x3_f32(input) [9*Cin rows, tap-major] or a = rfn_tap_scatter_f32(grad) [9*Cout rows].
 * Kernel choice (same arithmetic, same result up to summation order): F*HW >= 100000 pixels, HW % 32 == 0 and
 * Nc % 256 == 0 with M >= 192 or M <= 64 (grouped form: G * F*HW >= 100000) -> the LDS-DMA ring kernel (raw fp32 rows HBM -> LDS by global_load_lds, split
 * at the fragment reads; RFN_WGRAD_DMA=0 disables it); otherwise the register-staged tilings.  Argument checks, here and
 * in the four 3x3 forms below, run in the order of their codes: -1 null pointer / size <= 0 / G outside 1..16, -2 pixel
 * counts and strides the 16-byte loads cannot take, -3 a misaligned operand (grouped: a null or misaligned pointer of
 * any group), -4 F * HW >= 2^31 - 4096; with F == 0 a call that passes them returns 0 and launches nothing. */
int rfn_gemm_wgrad_bf16x3(const float* a, long a_ns, int M, const float* b, long b_ns, int Nc, float* gw, int F, int HW,
                          rfn_stream_t stream);
/* G (<= 16) gradients of ONE shape in one launch (the K steps of a flow level: one tail of atomics instead of K): a, b,
 * gw are host arrays of G device pointers; strides and sizes are shared. */
int rfn_gemm_wgrad_grouped_bf16x3(const float* const* a, long a_ns, int M, const float* const* b, long b_ns, int Nc,
                                  float* const* gw, int G, int F, int HW, rfn_stream_t stream);
/* label query for both (G = 0: rfn_gemm_wgrad_bf16x3) */
const char* rfn_gemm_wgrad_kernel_label_bf16x3(int M, int Nc, long a_ns, long b_ns, int G, int F, int HW);
/* out[n][tap*Cin+ci][y][x] = in[n][ci][y+dy-1][x+dx-1] (0 outside); two-source input; out dense [N,9*Cin,H,W]. */
/* 3x3 (pad 1) weight gradient without the im2col buffer (W % 8 == 0): gw[Cout][9*(C1+C2)] += sum over frames and
 * pixels of g[co][px] * in[ci][px + tap], column index ci*9 + tap: gw is the torch weight layout [Cout][Cin][3][3].
 * gw must be zeroed by the caller (split over pixel stages, atomic combine). */
int rfn_conv3x3_wgrad_implicit_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                      const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                      rfn_stream_t stream);
int rfn_conv3x3_wgrad_implicit_grouped_bf16x3(const float* const* g, long g_ns, int Cout, const float* const* in1,
                                              long in1_ns, int C1, const float* const* in2, long in2_ns, int C2,
                                              float* const* gw, int G, int F, int H, int W, rfn_stream_t stream);
/* label query for both (G = 0: the ungrouped entry point) */
const char* rfn_conv3x3_wgrad_implicit_kernel_label_bf16x3(int Cout, long g_ns, int G, int F, int H, int W);
/* The same for a 3x3 conv with FEW outputs (Cin -> C, the last conv of a coupling net), roles swapped and taps mirrored:
 * the Cin rows of the conv's input h are the big operand, the C gradient planes g are shifted while staging -- no
 * tap-scattered copy of g in memory.  gwT[Cin][C*9] += sum over frames and pixels of h[ci][q] * g[co][q - tap], column
 * index co*9 + tap: gwT is the TRANSPOSE [Cin][C][3][3] of the torch layout; zeroed by the caller.  W % 8 == 0.
 * (The narrow column tiles of the ring kernel start
 * rfn_wgrad_split_workgroups' count with 512 in place of 256: two workgroups per CU.) */
int rfn_conv3x3_wgrad_mirrored_bf16x3(const float* h, long h_ns, int Cin, const float* g, long g_ns, int C, float* gwT,
                                      int F, int H, int W, rfn_stream_t stream);
int rfn_conv3x3_wgrad_mirrored_grouped_bf16x3(const float* const* h, long h_ns, int Cin, const float* const* g, long g_ns,
                                              int C, float* const* gwT, int G, int F, int H, int W, rfn_stream_t stream);
/* label query for both (G = 0: the ungrouped entry point); "" when the shape has no mirrored route */
const char* rfn_conv3x3_wgrad_mirrored_kernel_label_bf16x3(int Cin, long h_ns, int C, int G, int F, int H, int W);
/* The two forms above on maps whose rows are shorter than a staging unit of 8 pixels, which they refuse: W == 4 with an
 * even H (a unit is two image rows of one frame) and H == W == 2 (a unit is two consecutive frames; F may be odd).
 * rfn_conv3x3_wgrad_rows*: the arguments, checks, codes and output layout of rfn_conv3x3_wgrad_implicit*;
 * rfn_conv3x3_wgrad_rows_mirrored*: those of rfn_conv3x3_wgrad_mirrored*.  -2 for every other (H, W); the label
 * queries answer "" there. */
int rfn_conv3x3_wgrad_rows_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                  const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                  rfn_stream_t stream);
int rfn_conv3x3_wgrad_rows_grouped_bf16x3(const float* const* g, long g_ns, int Cout, const float* const* in1,
                                          long in1_ns, int C1, const float* const* in2, long in2_ns, int C2,
                                          float* const* gw, int G, int F, int H, int W, rfn_stream_t stream);
const char* rfn_conv3x3_wgrad_rows_kernel_label_bf16x3(int Cout, long g_ns, int G, int F, int H, int W);
int rfn_conv3x3_wgrad_rows_mirrored_bf16x3(const float* h, long h_ns, int Cin, const float* g, long g_ns, int C,
                                           float* gwT, int F, int H, int W, rfn_stream_t stream);
int rfn_conv3x3_wgrad_rows_mirrored_grouped_bf16x3(const float* const* h, long h_ns, int Cin, const float* const* g,
                                                   long g_ns, int C, float* const* gwT, int G, int F, int H, int W,
                                                   rfn_stream_t stream);
const char* rfn_conv3x3_wgrad_rows_mirrored_kernel_label_bf16x3(int Cin, long h_ns, int C, int G, int F, int H, int W);
/* 3x3 (pad 1) weight gradient of a conv whose BOTH channel counts are small (Cout <= 128, C1 + C2 <= 128; W % 8 == 0),
 * whichever is larger: the arguments, codes, accumulation into the caller's zeroed gw and the output layout
 * [Cout][Cin][3][3] of rfn_conv3x3_wgrad_implicit_bf16x3.  The unit of work is a band of R image rows of one frame (R
 * divides H, R * W % 16 == 0): a persistent workgroup stages the band of g and of the input (with its halo rows) once
 * per band, split to bf16 (hi, lo), the three x shifts as three copies in LDS; every tap is an LDS address.  Columns
 * are split by whole input channels over blockIdx.y, rows beyond 64 over blockIdx.z; one tail of float atomics per
 * launch.  -2 where rfn_conv3x3_wgrad_band_supported answers 0 (no band of the map fits the LDS of half a CU, W % 8
 * != 0, a channel count above 128); the label query answers "" there.  The entry point takes every supported shape;
 * the size rule is rfn_hip.ops.wgrad_plan's.  rfn_conv3x3_wgrad_band_geometry: what a launch would use, {R, channels
 * per column block, grid x, y, z, LDS bytes}, without a device. */
int rfn_conv3x3_wgrad_band_supported(int Cout, int Cin, int H, int W);
int rfn_conv3x3_wgrad_band_bf16x3(const float* g, long g_ns, int Cout, const float* in1, long in1_ns, int C1,
                                  const float* in2, long in2_ns, int C2, float* gw, int F, int H, int W,
                                  rfn_stream_t stream);
const char* rfn_conv3x3_wgrad_band_kernel_label_bf16x3(int Cout, int Cin, int F, int H, int W);
int rfn_conv3x3_wgrad_band_geometry(int Cout, int Cin, int F, int H, int W, long long* out6);
/* K split of a GROUPED launch of the LDS-DMA ring kernels (gemm_wgrad_dma_kernel, gemm_wgrad_dma_impl_kernel), as
 * host-only queries that launch nothing and run the very functions the kernels and launchers run.  The unit of work is
 * the flat stage space of one output tile: G * n_stages stages (n_stages = F * HW / 32), group g owning
 * [g * n_stages, (g + 1) * n_stages).  rfn_wgrad_split_workgroups: the workgroups Wt a launch starts per tile,
 * min(256 / tiles, G * n_stages / 8), at least 1.  rfn_wgrad_split_parts: workgroup w of Wt owns the stages
 * [w T / Wt, (w + 1) T / Wt) of T = G * n_stages and processes them as parts that never cross a group; writes up to
 * max_parts triples (group, first stage within the group, count) in processing order and returns the number of parts
 * of w (0 for an empty range; negative: argument error). */
int rfn_wgrad_split_workgroups(int tiles, int G, int n_stages);
int rfn_wgrad_split_parts(int G, int n_stages, int Wt, int w, long long* parts, int max_parts);
int rfn_im2col3x3_f32(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2, float* out, int N,
                      int H, int W, rfn_stream_t stream);

/* number of floats of a packed weight buffer for (Cout, Cin, ks) */
long rfn_packed_weight_size(int Cout, int Cin, int ks);
/* Pack torch-layout weights w[Cout][Cin][ks][ks] for rfn_conv2d_fwd_f32.
 * transpose_flip = 0: forward conv.  transpose_flip = 1: the data-gradient conv (roles of Cin/Cout swapped, taps
 * mirrored), i.e. the packed buffer then describes a conv with Cin'=Cout inputs and Cout'=Cin outputs. */
int rfn_pack_conv_weight_f32(const float* w, float* wpk, int Cout, int Cin, int ks, int transpose_flip,
                             rfn_stream_t stream);

/* weight gradient, tap-major: gwt[ks*ks][Cout][Cin] += Σ_{n,y,x} g[n,co,y,x] · in[n,ci,y+dy,x+dx]  (two-source
 * input as above).  gwt is ACCUMULATED into with float atomics (caller zeroes it); tap-major so that one MFMA
 * accumulator register is a contiguous 128-byte atomic segment. */
int rfn_conv2d_wgrad_f32(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                         const float* g, long g_ns, int Cout, float* gwt, int N, int H, int W, int ks,
                         rfn_stream_t stream);
const char* rfn_conv2d_wgrad_kernel_label_f32(int ks, int Cin, int Cout, int H, int W); /* label query */
/* gw[Cout][Cin][ks][ks] (torch layout) = (accumulate ? gw : 0) + transpose of gwt[ks*ks][Cout][Cin]. */
int rfn_wgrad_finish_f32(const float* gwt, float* gw, int Cout, int Cin, int ks, int accumulate, rfn_stream_t stream);

/* Tap-expanded form of a 3x3 convolution with very few output channels (Conv2dZeros at the shallow flow levels,
 * glow_modules.py:106-121 with Cout = 4 / 8): the conv runs as a 1x1 rfn_conv2d_fwd_f32 to 9*C channels
 * P[n][tap*C+co] (dense [N,9C,H,W]); rfn_tap_gather_f32 then forms
 *   o[n][co][y][x] = (Σ_tap P[n][tap*C+co][y+dy-1][x+dx-1] + bias[co]) * exp(3*logs[co])   (bias/logs both NULL: plain sum).
 * rfn_tap_scatter_f32 is the adjoint data movement used for the weight gradient:
 *   Gs[n][tap*C+co][y][x] = g[n][co][y-dy+1][x-dx+1] (0 outside); a 1x1 rfn_conv2d_wgrad_f32 of Gs gives gW[co][ci][tap].
 * All tensors dense NCHW. */
int rfn_tap_gather_f32(const float* P, const float* bias, const float* logs, float* o, int N, int C, int H, int W,
                       rfn_stream_t stream);
int rfn_tap_scatter_f32(const float* g, float* Gs, int N, int C, int H, int W, rfn_stream_t stream);

/* backward through  y = act((u + b[c]) * exp(l[c]))  (ep_mode 1) or  y = (u + b[c]) * exp(3 l[c])  (ep_mode 2),
 * given y (saved forward output) and gy:   gu (may alias gy) ;  gb[c] += ...;  gl[c] += ...  (accumulated). */
int rfn_conv_epilogue_bwd_f32(const float* y, long y_ns, const float* gy, long gy_ns, float* gu, long gu_ns,
                              const float* logs, float* gb, float* gl, int N, int C, int HW, int ep_mode, int act,
                              rfn_stream_t stream);

/* ---- a5  AffineCoupling.forward, everything after the coupling net  (glow_modules.py:276-291):
 * o = NN output [N,C,HW] with shift = o[:,0::2], s = o[:,1::2];  ls = clamp(s) (clamp_type 0 realnvp:
 * scale[c]*tanh(s)+scale_shift[c]; 1 glow: log sigmoid(s+2); 2 softclamp: 2.5*0.636*atan(s/2.5); 3 none);
 * forward (reverse=0): z2 <- (z2 + shift) * exp(ls), logdet[n] += Σ ls;  reverse=1: z2 <- z2*exp(-ls) - shift,
 * logdet[n] -= Σ ls.   z2 = channels [C/2, C) of z, updated IN PLACE.  logdet may be NULL. */
int rfn_affine_coupling_f32(float* z, long z_ns, const float* o, long o_ns, const float* scale,
                            const float* scale_shift, float* logdet, int clamp_type, int reverse, int N, int C, int HW,
                            rfn_stream_t stream);
/* backward of the forward direction.  zout = output of the forward (z1 | z2'), gout = grad wrt it, glogdet[N] = grad
 * wrt logdet.  Writes gz2 into channels [C/2,C) of gz (channels [0,C/2) of gz are NOT touched), go [N,C,HW] (grad wrt
 * the NN output) and accumulates gscale[C/2], gscale_shift[C/2]. */
int rfn_affine_coupling_bwd_f32(const float* zout, long zout_ns, const float* o, long o_ns, const float* gout,
                                long gout_ns, const float* glogdet, const float* scale, const float* scale_shift,
                                float* gz, long gz_ns, float* go, long go_ns, float* gscale, float* gscale_shift,
                                int clamp_type, int N, int C, int HW, rfn_stream_t stream);

/* ---- a7/a8  Gaussian log-likelihood reductions  (glow_modules.py:358-365, glow.py:135-140):
 * logp[n] += Σ_{c,p} log N(z[n,c,p]; mean, std).
 *   layout 0 ("cross", Split2d): mean = o[:,2c], raw = o[:,2c+1];  layout 1 ("split", base prior): mean = o[:,c],
 *   raw = o[:,Cz+c].   std_mode 0: softplus(raw)+1e-8 ; 1: exp(raw).   o has 2*Cz channels, z has Cz. */
int rfn_gauss_logp_f32(const float* z, long z_ns, const float* o, long o_ns, float* logp, int layout, int std_mode,
                       int N, int Cz, int HW, rfn_stream_t stream);
/* backward: gz (written) and go (written) from glogp[N]. */
int rfn_gauss_logp_bwd_f32(const float* z, long z_ns, const float* o, long o_ns, const float* glogp, float* gz,
                           long gz_ns, float* go, long go_ns, int layout, int std_mode, int N, int Cz, int HW,
                           rfn_stream_t stream);
/* reverse / sampling (glow_modules.py:366-369, glow.py:153-154): z = mean + std*temperature*eps. */
int rfn_gauss_sample_f32(const float* o, long o_ns, const float* eps, float* z, long z_ns, float temperature, int layout,
                         int std_mode, int N, int Cz, int HW, rfn_stream_t stream);
/* the same with one temperature per frame: z[n] = mean + std*temperature_rows[n]*eps, temperature_rows a device array of
 * N floats.  The same kernel as rfn_gauss_sample_f32 (the pointer selects the row's value, uniform per block), so rows
 * that hold the scalar's value give the scalar call's bits. */
int rfn_gauss_sample_rows_f32(const float* o, long o_ns, const float* eps, float* z, long z_ns,
                              const float* temperature_rows, int layout, int std_mode, int N, int Cz, int HW,
                              rfn_stream_t stream);

/* ---- a10  SRNN latent step of RFN.loss (RFN/RFN_new.py:167-184,206-207 with SimpleParamNet's chunk + softplus,
 * Utils/modules.py:240-244): enc, pri = [B, 2*Z*HW] outputs of the encoder / prior parameter convs (loc half | raw scale
 * half); ps = softplus(pri_raw), es = softplus(enc_raw), pm = pri_loc, em = enc_loc (+ pm when res_q);
 *   zt = pm + ps*eps_p,  zxt = em + es*eps_q,  kl = KL(N(em,es)||N(pm,ps)) element-wise,  em/es also returned.
 * ZHW = Z*H*W.  The backward takes the gradients of the five outputs (any may be NULL) and writes g_enc, g_pri; g_zt and
 * g_zxt are read with a row stride in floats (>= ZHW), so a channel slice of a wider gradient needs no copy. */
int rfn_latent_step_fwd_f32(const float* enc, const float* pri, const float* eps_p, const float* eps_q, float* zt,
                            float* zxt, float* kl, float* em, float* es, int B, int ZHW, int res_q, rfn_stream_t stream);
int rfn_latent_step_bwd_f32(const float* enc, const float* pri, const float* eps_p, const float* eps_q,
                            const float* g_zt, long g_zt_ns, const float* g_zxt, long g_zxt_ns, const float* g_kl,
                            const float* g_em, const float* g_es, float* g_enc, float* g_pri, int B, int ZHW, int res_q,
                            rfn_stream_t stream);

/* ---- VRNN baseline: the diagonal Gaussians of one time step, csrc/gauss_heads.hip  (VRNN/VRNN.py:203-213 + :223 in
 * `loss`, :383-394 + :419-420 in `elbo_importance_weighting`, :265-273 and :290-294 in `predict`: td.Normal of the
 * encoder and prior MLP outputs, both rsamples, td.kl_divergence, Normal.log_prob of each sample -- about twenty torch
 * launches per step).  All tensors [B, Z] contiguous; sigma = softplus(raw) as torch.nn.Softplus() computes it (raw itself
 * where raw > 20, else log1p(exp(raw))); nothing is added to sigma (this is not rfn_gauss_logp's +1e-8, nor
 * rfn_latent_step's pairing of halves).
 *   z_q = q_loc + sq*eps_q,  z_p = p_loc + sp*eps_p,  q_scale = sq,  p_scale = sp;
 *   with a = sq/sp, d = (q_loc - p_loc)/sp:   kl[b] = sum_j  (a^2 + d^2 - 1)/2 - (log sq - log sp);
 *   logq[b] = sum_j  -eps_q^2/2 - log sq - log(2 pi)/2,  logp[b] the same with p: the density at the OWN sample.
 * Every output pointer may be NULL.  eps_q NULL: no z_q and no logq; eps_p NULL: no z_p and no logp; q_loc, q_raw and eps_q
 * all NULL: the prior-only form of generation (z_p, p_scale, logp).  p_loc / p_raw are always needed.  -1: sizes below 1, a
 * missing p input, one of q_loc / q_raw without the other; -2: an output (backward: an upstream gradient, or eps_q) whose
 * inputs are missing; -3: a gradient row stride below Z.  Nothing is launched then.
 * Backward: the gradient of the formulas above, sigma recomputed, sigma'(raw) = logistic(raw) and exactly 1 above the
 * threshold.  g_zq / g_zp are read with a row stride in floats (>= Z), as rfn_latent_step_bwd_f32 reads its own; g_kl,
 * g_logq, g_logp are [B]; any upstream pointer may be NULL.  g_q_loc, g_q_raw, g_p_loc, g_p_raw are WRITTEN (g_q_* are NULL
 * exactly when q_loc is).
 * One wavefront per row, four rows per workgroup; lane l adds the terms of elements l, l + 64, ... in index order and the
 * 64 lane sums are combined by a fixed xor butterfly (32, 16, ..., 1): no atomics, no LDS memory, a row's bits depend on
 * that row alone (not on B or the grid).  Any B >= 1, Z >= 1; one launch, no allocation: capturable. */
int rfn_gauss_heads_fwd_f32(const float* q_loc, const float* q_raw, const float* p_loc, const float* p_raw,
                            const float* eps_q, const float* eps_p, float* z_q, float* z_p, float* q_scale,
                            float* p_scale, float* kl, float* logq, float* logp, int B, int Z, rfn_stream_t stream);
int rfn_gauss_heads_bwd_f32(const float* q_loc, const float* q_raw, const float* p_loc, const float* p_raw,
                            const float* eps_q, const float* eps_p, const float* g_zq, long g_zq_ns, const float* g_zp,
                            long g_zp_ns, const float* g_kl, const float* g_logq, const float* g_logp, float* g_q_loc,
                            float* g_q_raw, float* g_p_loc, float* g_p_raw, int B, int Z, rfn_stream_t stream);

/* ---- SVG baseline: one torch.nn.LSTMCell call, csrc/lstm_cell.hip  (SVG/SVG.py:131,149 and :163,185 of the reference:
 * every layer of frame_predictor, posterior and prior).  All tensors contiguous float32: x [B, I], h [B, H], c [B, H],
 * w_ih [4H, I], w_hh [4H, H], b_ih [4H], b_hh [4H]; rows gH .. gH+H-1 belong to gate g, g = 0..3 = i, f, g, o.
 *   pre_g[b,j] = sum_k x[b,k] w_ih[gH+j,k] + sum_k h[b,k] w_hh[gH+j,k] + b_ih[gH+j] + b_hh[gH+j]
 *   i = sigmoid(pre_i), f = sigmoid(pre_f), g = tanh(pre_g), o = sigmoid(pre_o);  c' = f c + i g,  h' = o tanh(c')
 * fwd WRITES h_out [B, H] = h', c_out [B, H] = c' and gates [B, 4H] = (i | f | g | o), which the backward reads; the
 * pre-activations never reach memory.  The products run on the float32-input MFMA 16x16x4 (exact float32 products, one
 * fma chain per output): a workgroup of four waves owns a 16-row x 16-unit tile, the k range is cut into chunks of 16
 * (those of x first, then those of h), wave w adds the chunks w, w + 4, ... for all four gates, the four partial sums are
 * added in wave order, then b_ih, then b_hh.  The order of summation of an output depends on I and H alone.  Operands are
 * read 16 bytes at a time where I (H) is a multiple of 4 and the bases are 16-byte aligned, else as single floats, in the
 * same order.
 * bwd, with the upstreams gh = dL/dh' and gc = dL/dc' (either may be NULL = zero) and t = tanh(c'):
 *   gct = gc + gh o (1 - t^2);  d_i = gct g i(1-i),  d_f = gct c f(1-f),  d_g = gct i (1-g^2),  d_o = gh t o(1-o)
 * WRITES D [B, 4H] = (d_i | d_f | d_g | d_o), g_c [B, H] = gct f and g_bias [4H] = sum_b D[b,:] (the gradient of b_ih and
 * of b_hh): thread (unit, row group rg of 16) adds the rows rg, rg + 16, ... in order and the 16 sums are added in
 * row-group order -- no atomics.  The four matrix products of the backward (D w_ih, D w_hh, D^T x, D^T h) are the
 * caller's.  Any B, I, H >= 1 (I, H <= 2^28; ceil(B/16) * ceil(H/16) tiles < 2^31, more
 * than any memory holds); one launch each, no allocation: capturable.  Bad sizes return
 * -1, a missing required pointer -2; nothing is launched then. */
int rfn_lstm_cell_fwd_f32(const float* x, const float* h, const float* c, const float* w_ih, const float* w_hh,
                          const float* b_ih, const float* b_hh, float* h_out, float* c_out, float* gates, int B, int I,
                          int H, rfn_stream_t stream);
int rfn_lstm_cell_bwd_f32(const float* gh, const float* gc, const float* gates, const float* c, const float* c_out,
                          float* D, float* g_c, float* g_bias, int B, int H, rfn_stream_t stream);

/* ---- a10  the per-timestep parameter nets (SimpleParamNet, Utils/modules.py:216-244, called once per frame by
 * RFN.loss, RFN/RFN_new.py:167-179) on small maps: a 3x3 / pad 1 convolution on an H x W <= 16 pixel map is the dense
 * product out[b][(co,po)] = bias[co] + sum x[b][(ci,pi)] * w[co][ci][tap(po,pi)] over NCHW-contiguous samples.
 * rfn_smallmap_pack_bf16x3 writes w [Cout][Cin][3][3] in MFMA fragment order, split into bf16 (hi, lo), for the forward
 * product (transpose 0: K = Cin*HW, N = Cout*HW) or the data gradient (transpose 1: K = Cout*HW, N = Cin*HW);
 * rfn_smallmap_packed_size gives the buffer size in bytes.  rfn_smallmap_dense_bf16x3: out[B][N] = a'[B][K] * packed
 * (+ bias[n / HW] + add[B][N], each optional, then leaky_relu(slope_out) when act_out), where a' = a, or a * (y > 0 ? 1 : slope_in) when y is given
 * (backward of an in-place leaky_relu whose result is y); a_out (optional) receives a'.  K % 8 == 0. */
long rfn_smallmap_packed_size(int Cout, int Cin, int H, int W, int transpose);
int rfn_smallmap_pack_bf16x3(const float* w, int Cout, int Cin, int H, int W, int transpose, float* packed,
                             rfn_stream_t stream);
/* The same for n matrices in ceil(n / 64) launches: host array of descriptors (the host hands over the packs a step asks
 * for back to back -- a recurrent net's layers, a ConvLSTM's two weight halves -- in one call; rfn_smallmap_pack_bf16x3
 * is the one-descriptor form of this call). */
typedef struct {
    const float* w;   /* [Cout][Cin][3][3] */
    float* packed;    /* rfn_smallmap_packed_size(Cout, Cin, H, W, transpose) bytes, 16-byte aligned */
    int Cout, Cin, H, W, transpose, pad_;
} rfn_smallmap_pack_desc;
int rfn_smallmap_pack_batched_bf16x3(const void* descs_host, int n, rfn_stream_t stream);
int rfn_smallmap_dense_bf16x3(const float* a, const float* y, float slope_in, const float* packed, const float* bias,
                              const float* add, int act_out, float slope_out, float* out, float* a_out, int B, int K, int N,
                              int HW, rfn_stream_t stream);

/* Two rfn_smallmap_dense_bf16x3 products (suffix 0 / 1) in one launch: the encoder and the prior layer of a
 * timestep (RFN_new.py:167-179) have no data dependence on each other.  Same B and HW; K, N per product. */
int rfn_smallmap_dense_pair_bf16x3(const float* a0, const float* y0, float slope_in0, const float* packed0,
                                   const float* bias0, const float* add0, int act_out0, float slope_out0, float* out0,
                                   float* a_out0, int K0, int N0, const float* a1, const float* y1, float slope_in1,
                                   const float* packed1, const float* bias1, const float* add1, int act_out1,
                                   float slope_out1, float* out1, float* a_out1, int K1, int N1, int B, int HW,
                                   rfn_stream_t stream);

/* The same dense product behind the interface of rfn_conv2d_fwd_bf16x3 (ks = 3 implied): N frames of an H x W <= 16
 * map, two-source input, ep_mode 0-3, output channels split at cout_split; acc1 is a bit mask (1: add into out1, 2: add
 * into out2).  `packed` from
 * rfn_smallmap_pack_bf16x3 of the [Cout][C1+C2][3][3] weight (transpose 0), or transpose 1 of the FORWARD weight for a
 * data gradient.  (C1*H*W) % 8 == 0 and ((C1+C2)*H*W) % 8 == 0.  Used for the coupling convolutions of the two deepest
 * flow levels, where a launch is a few thousand pixels against megabytes of weights. */
int rfn_smallmap_conv_bf16x3(const float* in1, long in1_ns, int C1, const float* in2, long in2_ns, int C2,
                             const float* packed, float* out1, long out1_ns, float* out2, long out2_ns, int Cout,
                             int cout_split, int acc1, int N, int H, int W, int ep_mode, const float* p0,
                             const float* p1, int act, rfn_stream_t stream);

/* ---- callers of the path (VGG extractor / upscaler, Utils/modules.py:43-213): BatchNorm2d (training mode) + the
 * activation that follows it on a step-major time-batched tensor x [S*B, C, HW] with the statistics of EACH step's B
 * samples, as the reference's per-timestep calls compute them (RFN_new.py:126-128,191-194).  mean / var (biased) are
 * [S*C]; act: 0 none, 1 relu, 2 leaky_relu(slope), 3 tanh; gamma / beta may both be NULL.  Backward: g' = g*act'(u) with u = xhat*gamma + beta recomputed from x (the output is not read),
 * sg = sum g', sgx = sum g'*xhat per (step, channel), gx = gamma*rstd*(g' - sg/n - xhat*sgx/n). */
/* One BatchNorm layer of the time-batched extractor / upscaler in two launches each way.  Forward: partial sums + apply;
 * the apply kernel derives the moments from the partial sums, writes mean / var [S*C] (kept for the backward) and applies
 * the S running-statistics updates of the reference's step-wise calls in closed form: run <- decay*run + sum_s
 * coef[s]*stat[s] (run_mean / run_var [C] both or neither, coef for the mean and coef_u for the unbiased variance are [S]
 * device arrays, decay = (1-momentum)^S); num_batches_tracked (int64, optional) += S.
 * Backward: per-step partial sums + apply; ggamma / gbeta [C] (both or neither) are written.  acc / sums = scratch of
 * rfn_stepbn_scratch_floats(S, B, C) floats (no zeroing needed: no atomics, results are deterministic). */
long rfn_stepbn_scratch_floats(int S, int B, int C);
int rfn_stepbn_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* var, float* acc,
                       float* run_mean, float* run_var, const float* coef, const float* coef_u, float decay,
                       long long* num_batches_tracked, int S, int B, int C, int HW, float eps, int act, float slope,
                       rfn_stream_t stream);
int rfn_stepbn_bwd_f32(const float* x, const float* gamma, const float* beta, const float* g, const float* mean,
                       const float* var, float* sums, float* gx, float* ggamma, float* gbeta, int S, int B, int C, int HW,
                       float eps, int act, float slope, int stage, int world, rfn_stream_t stream);
/* Synchronised BatchNorm over `world` data-parallel ranks (same mathematics as one process on the
 * global batch): forward = rfn_stepbn_fwd_f32 for the local moments, the caller combines the ranks' moments, then
 * rfn_stepbn_apply_f32 normalises with the GIVEN statistics; backward = rfn_stepbn_bwd_f32 with stage 1 (partial sums
 * only), the caller adds `sums` over the ranks, then stage 2 (apply; gx uses the global means of g' and g'*xhat, the
 * parameter gradients are the sums divided by `world`: the reducer's rank average then gives the global-batch gradient).
 * stage 0 / world 1 = the single-process behaviour. */
int rfn_stepbn_apply_f32(const float* x, const float* gamma, const float* beta, float* y, const float* mean,
                         const float* var, int S, int B, int C, int HW, float eps, int act, float slope,
                         rfn_stream_t stream);
/* Host-only label query: "stepbn ny=.. stats=vec|scalar apply=vec4|vec1 grid=.. sweeps=..".  ny = workgroups per (step,
 * channel) of the stats / reduce kernel (= rfn_stepbn_scratch_floats / (2*S*C)); grid = streaming workgroups of the
 * apply kernel, sweeps = the most grid-stride iterations of one.  `aligned` is a bit mask the caller derives from the
 * pointers it will pass: bit 0 = every pointer the stats (x) or, with bwd, the reduce kernel (x, g) tests is 16-byte
 * aligned; bit 1 = the same for the apply kernel (x, y; with bwd x, g, gx). */
const char* rfn_stepbn_kernel_label(int S, int B, int C, int HW, int aligned, int bwd);
/* Per-step BatchNorm + activation + MaxPool2d(2, 2) (the extractor's conv -> norm -> act -> pool): x [S*B, C, H, W] with
 * even H and W (odd: argument error), p / gp [S*B, C, H/2, W/2].  Forward: the statistics launch of rfn_stepbn_fwd_f32,
 * then ONE apply launch that reads x and writes only p; mean / var / running statistics / num_batches_tracked as there.
 * A window's winner follows max_pool2d: the ACTIVATED values in the order (0,0), (0,1), (1,0), (1,1), a candidate
 * replacing the best when it is larger or NaN; p is bit-equal to rfn_stepbn_fwd_f32 followed by max_pool2d.
 * Backward from the POOLED gradient: the reduce kernel recomputes every winner from x and sums g' = gp act'(u_winner)
 * and g' xhat_winner into the same [ny][S*C] partial rows (scratch of rfn_stepbn_scratch_floats, no atomics, nothing to
 * zero); the apply kernel writes gx = gamma rstd (g' [winner] - k1 - xhat k2) at all four positions of a window and the
 * parameter gradients.  stage / world as rfn_stepbn_bwd_f32.  No index map and no full-resolution gradient exist. */
int rfn_stepbn_pool_fwd_f32(const float* x, const float* gamma, const float* beta, float* p, float* mean, float* var,
                            float* acc, float* run_mean, float* run_var, const float* coef, const float* coef_u,
                            float decay, long long* num_batches_tracked, int S, int B, int C, int H, int W, float eps,
                            int act, float slope, rfn_stream_t stream);
int rfn_stepbn_pool_bwd_f32(const float* x, const float* gamma, const float* beta, const float* gp, const float* mean,
                            const float* var, float* sums, float* gx, float* ggamma, float* gbeta, int S, int B, int C,
                            int H, int W, float eps, int act, float slope, int stage, int world, rfn_stream_t stream);
/* Host-only label query: "stepbn_pool ny=.. stats=vec|scalar apply=vec4|vec1 grid=.. sweeps=..".  `aligned` as for
 * rfn_stepbn_kernel_label: bit 0 = x (the statistics kernel) or, with bwd, x and gp (the reduce kernel) are 16-byte
 * aligned; bit 1 = the same for the apply kernel (x, p; with bwd x, gp, gx).  The pooled kernels take 16-byte accesses
 * when W % 4 == 0 as well (a unit = two rows x four columns = two windows), else one window per thread with scalar
 * accesses; the statistics kernel is the unpooled one (H*W % 4 == 0 always holds here).  "unsupported": odd H or W, a
 * size < 1, or 2^31 elements and more. */
const char* rfn_stepbn_pool_kernel_label(int S, int B, int C, int H, int W, int aligned, int bwd);

/* ---- nearest 2x up-sampling + channel concatenation (the upscaler's NearestUp2x -> cat((x, skip), 1)), one launch each
 * way.  x [N, Cx, h, w] and skip [N, Cs, 2h, 2w] with frame strides x_ns / skip_ns (floats; the per-frame block dense),
 * out [N, Cx+Cs, 2h, 2w] dense.  Backward: gx [N, Cx, h, w] = the 2x2 block sums of the first Cx channels of
 * g [N, *, 2h, 2w], read in place through its frame stride g_ns (each sum formed in fp64 and rounded once); the skip's
 * gradient is the view g[:, Cx:].  16-byte accesses when w is even, every pointer 16-byte aligned and every frame stride
 * a multiple of 4; else one element per thread.  Label: "up2x_cat[_bwd] access=vec4|vec1 grid=.. sweeps=..", `aligned`
 * = that condition on pointers and strides. */
int rfn_up2x_cat_f32(const float* x, long x_ns, const float* skip, long skip_ns, float* out, int N, int Cx, int Cs, int h,
                     int w, rfn_stream_t stream);
int rfn_up2x_cat_bwd_f32(const float* g, long g_ns, float* gx, int N, int Cx, int h, int w, rfn_stream_t stream);
const char* rfn_up2x_cat_kernel_label(int N, int Cx, int Cs, int h, int w, int aligned, int bwd);

/* ---- BatchNormFlow (Flow/glow_modules.py:56-104), the flow normalisation of --flow_norm batchnorm, on a step-major
 * time-batched tensor x [S*B, E] with E = C*H*W: log_gamma, beta, run_mean, run_var are [E] (one value per channel AND
 * pixel), and the statistics of each step's B rows are taken on their own, as the reference's per-timestep calls take
 * them (glow_modules.py:76-79: mean = mean_b x, var = mean_b (x - mean)^2 + eps, eps INSIDE var also where the log-det
 * reads it).  Forward, training (glow_modules.py:93-98): z = exp(log_gamma)*(x - mean)/sqrt(var) + beta, dl[s] = sum_e
 * (log_gamma - 0.5 log var[s]) to be added to the log-det of every row of step s; mean / var [S*E] are kept for the
 * backward.  run_mean / run_var (both or neither) receive the S updates of glow_modules.py:81-87 in closed form, run <-
 * decay*run + sum_s coef[s]*stat[s] with coef_mean / coef_var [S] device arrays; the momentum weights the OLD value, so
 * decay = m^S and coef[s] = (1-m) m^(S-1-s).
 * Backward, given gz [S*B, E] and gdl [S] (may be NULL = 0), with xhat = (x - mean)/sqrt(var), rstd = 1/sqrt(var),
 * g' = gz*exp(log_gamma): gx = rstd*(g' - mean_b g' - xhat*mean_b(g' xhat)) - gdl[s]*xhat*rstd/B (the log-det depends on
 * the data through var), g_log_gamma = sum_{s,b} g' xhat + sum_s gdl[s], g_beta = sum_{s,b} gz.
 * scratch = rfn_bnflow_scratch_floats(S, B, E, bwd) floats (bwd = 0, the forward: log-det partials, S*ceil(E/64); bwd = 1,
 * the backward: per-step gradient partials, 2*S*E; no
 * zeroing needed: no atomics, every sum is taken in a fixed order and the results repeat bit for bit).  Two launches each.
 * 16-byte accesses when E % 4 == 0 and every tensor pointer is 16-byte aligned, 4-byte accesses otherwise. */
long rfn_bnflow_scratch_floats(int S, int B, int E, int bwd);
int rfn_bnflow_fwd_f32(const float* x, const float* log_gamma, const float* beta, float* z, float* mean, float* var,
                       float* dl, float* scratch, float* run_mean, float* run_var, const float* coef_mean,
                       const float* coef_var, float decay, int S, int B, int E, float eps, rfn_stream_t stream);
int rfn_bnflow_bwd_f32(const float* x, const float* log_gamma, const float* gz, const float* gdl, const float* mean,
                       const float* var, float* gx, float* g_log_gamma, float* g_beta, float* scratch, int S, int B,
                       int E, rfn_stream_t stream);
/* The map with GIVEN statistics (glow_modules.py:90-103: eval mode, and the reverse direction in any mode) on N rows, one
 * launch: forward y = exp(log_gamma)/sqrt(run_var)*(x - run_mean) + beta, dl[0] = sum_e (log_gamma - 0.5 log run_var);
 * reverse y = (x - beta)*sqrt(run_var)/exp(log_gamma) + run_mean, dl[0] = minus that sum (bit for bit). */
int rfn_bnflow_apply_f32(const float* x, const float* log_gamma, const float* beta, const float* run_mean,
                         const float* run_var, float* y, float* dl, int N, int E, int reverse, rfn_stream_t stream);

/* ---- Mixture of discretized logistics, the likelihood of the SRNN baseline (Utils/discretize_logits.py; DESIGN.md
 * section 19 is the definition).  x [N,C,HW] in [-1,1], C in {1,3}; l [N,Cl,HW] with Cl = M (1 + P C), P = 3 for C = 3
 * (mean, log-scale, coefficient) and 2 for C = 1; any M >= 1; dense fp32 NCHW.  Channel m is the mixture logit of
 * component m, channel M + (c P + j) M + m parameter j of colour channel c.  For C = 3 the tanh of the coefficients of
 * colour rows 0, 1, 2 enter as mean_1 += t0 x_0, mean_2 += t1 x_0 + t2 x_1.
 * rfn_mol_nll_fwd: nll_pix [N,HW] = -log sum_m softmax(logit)_m prod_c P(x_c | m) with log-scales clamped at -7, bins of
 *   +-1/255, the edge branches for x < -0.999 and x > 0.999, log(cdf_delta) where cdf_delta > 1e-5 and the mid-bin density
 *   (log_pdf_mid - log 127.5) otherwise; nll [N] = the sum over a frame's pixels: each workgroup's 256 pixels (all of
 *   one frame), then the rfn_mol_part_floats(N, HW) / N partials of the frame in index order -- no atomics, and the bits
 *   of a frame's sum depend on that frame alone.  lse [N,HW] = log sum_m exp(logit_m + sum_c log P(x_c | m)), kept for
 *   the backward.  part: rfn_mol_part_floats(N, HW) floats of scratch.  Two launches.
 * rfn_mol_nll_bwd: dl [N,Cl,HW] = up * d nll_pix / d l, up [N] (up_per_pixel = 0) or [N,HW] (1); recomputed from x, l and
 *   the forward's lse (the responsibility of a component is exp(its term - lse): exactly 1 for M = 1).  A selected branch alone receives gradient; none passes a binding clamp (log-scale < -7).
 *   One launch; every element of dl is written.
 * rfn_mol_sample: u_mix [N,HW,M], u_x [N,HW,C] uniforms in (0,1); component argmax_m(logit_m - log(-log u_mix_m)), the
 *   lowest index on a tie; x_c = clamp(mean_c + exp(max(log-scale_c, -7)) (log u_c - log(1 - u_c)) + the coefficient
 *   terms on the clamped x_0, x_1, -1, 1); out [N,C,HW], not rounded to 8 bits.  One launch. */
long rfn_mol_part_floats(int N, int HW);
int rfn_mol_nll_fwd(const float* x, const float* l, float* nll_pix, float* lse, float* nll, float* part, int N, int C, int M,
                    int HW, rfn_stream_t stream);
int rfn_mol_nll_bwd(const float* x, const float* l, const float* lse, const float* up, int up_per_pixel, float* dl, int N,
                    int C, int M, int HW, rfn_stream_t stream);
int rfn_mol_sample(const float* l, const float* u_mix, const float* u_x, float* out, int N, int C, int M, int HW,
                   rfn_stream_t stream);
/* The sampler with addressed uniforms (SRNN.predict_draws; DESIGN.md section 20 is the contract): what rfn_mol_sample
 * computes, by the same device function, on uniforms made inside the kernel from their address.  l [rows,Cl,HW], out
 * [rows,C,HW]; row i of a launch is draw first_draw + i / B of sequence first_seq + i % B (draw-major, as
 * rfn_keyed_normal_f32).  Block j of pixel p (the index inside the frame) is
 *   Philox4x64-10(key = (seed, (step << 32) | slot), counter = (j, p, seq, draw)),  slot 16 mixture, slot 17 colour
 * (rfn_keyed_normal_f32 owns slots 0..7, so no address is shared with it).  Uniform e of a pixel (e = m for the mixture,
 * e = c for the colour) is the 32-bit half e % 8 of block e / 8, the halves in the order high half of w0, low half of
 * w0, high half of w1, ...:
 *   u = min(max((2 (half >> 9) + 1) * 2^-24, 1e-5f), 1 - 1e-5f)
 * The numerator is an odd integer below 2^24: exact in fp32, never 0 or 1.  A value depends on (seed, step, slot,
 * sequence, draw, pixel, element) and on nothing else: not on rows, B, the grid or the other rows of the launch.
 * rows is a multiple of B >= 1; seed, step, first_seq, first_draw >= 0.  No atomics, no LDS, no scratch.  One launch.
 * rfn_mol_keyed_uniforms writes exactly those uniforms as u_mix [rows,HW,M] and u_x [rows,HW,C]:
 * rfn_mol_sample(l, u_mix, u_x) then equals rfn_mol_sample_keyed(l) bit for bit. */
int rfn_mol_sample_keyed(const float* l, float* out, int rows, int B, int C, int M, int HW, long seed, int step,
                         long first_seq, long first_draw, rfn_stream_t stream);
int rfn_mol_keyed_uniforms(float* u_mix, float* u_x, int rows, int B, int C, int M, int HW, long seed, int step,
                           long first_seq, long first_draw, rfn_stream_t stream);

/* ---- a9  ConvLSTMLayer.forward gate update  (Utils/modules.py:370-377): cc = conv output [N,4*Hc,HW] in gate order
 * i,f,o,g;  i=σ(cc_i+Wci∘c) f=σ(cc_f+Wcf∘c) g=tanh(cc_g) c'=f∘c+i∘g o=σ(cc_o+Wco∘c') h'=o∘tanh(c').
 * Wci/Wcf/Wco [Hc*HW] may be NULL (== 0, which is what the reference trains with).  gates [N,4*Hc,HW] receives the
 * post-nonlinearity i,f,o,g for the backward pass (may be NULL). */
/* Host-only label queries of the grid-stride launches above and below (answered by the host functions the launchers
 * call for their grids): "latent_step grid=.. sweeps=.." / "convlstm_gates grid=.. sweeps=..", sweeps = the most
 * grid-stride iterations of a thread; "unsupported" for sizes that launch nothing. */
const char* rfn_latent_step_kernel_label(int B, int ZHW);
const char* rfn_convlstm_gates_kernel_label(int N, int Hc, int HW);
int rfn_convlstm_gates_fwd_f32(const float* cc, const float* c_prev, long c_ns, const float* Wci, const float* Wcf,
                               const float* Wco, float* h_out, long h_ns, float* c_out, long co_ns, float* gates,
                               int N, int Hc, int HW, rfn_stream_t stream);
/* backward: from gh, gc_next (either may be NULL), saved gates, c_prev, c_out -> gcc [N,4Hc,HW], gc_prev.
 * The peephole terms enter the state gradients; gradients w.r.t. Wci/Wcf/Wco themselves are not produced (the
 * reference never trains them on a GPU: Utils/modules.py:385-393 creates them as non-leaf tensors). */
int rfn_convlstm_gates_bwd_f32(const float* gates, const float* c_prev, long c_ns, const float* c_out, long co_ns,
                               const float* gh, long gh_ns, const float* gc_next, long gcn_ns, const float* Wci,
                               const float* Wcf, const float* Wco, float* gcc, float* gc_prev, long gcp_ns, int N,
                               int Hc, int HW, rfn_stream_t stream);

/* ---- the optimizer of the training step  (RFN/trainer.py:96: torch.optim.Adam with its defaults; the arithmetic is
 * torch's: m <- m + (1-b1)(g - m), v <- b2 v + (1-b2) g^2, p <- p - lr/(1-b1^s) * m / (sqrt(v)/sqrt(1-b2^s) + eps), with
 * g += weight_decay*p first when weight_decay != 0) for ALL parameter tensors in one launch.  `table` and `chunks` are
 * DEVICE arrays built by the host: one rfn_adam_entry per tensor (s = t - step_offset is that tensor's step count, >= 1)
 * and one (tensor index, chunk index) int pair per workgroup, a chunk being rfn_adam_chunk_elems() consecutive elements.
 * p, m, v are updated in place; g is read only.  The hyper-parameters arrive as doubles (Python floats): 1 - beta and the
 * bias corrections are formed in double and rounded once, the per-element arithmetic is fp32. */
typedef struct rfn_adam_entry {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
    int step_offset;
    int flags; /* bit 0: this tensor's gradient is rank-local (see rfn_grad_sumsq_f32); 0 in tables built before it existed */
} rfn_adam_entry;
int rfn_adam_chunk_elems(void);
int rfn_adam_step_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int t, rfn_stream_t stream);

/* ---- guard of the Adam step: global gradient-norm clipping and "skip the step if the gradients are not finite", decided
 * on the device from the same `table` and `chunks` (no host read; sumsq -> [all-reduce of sumsq[1] under data parallelism]
 * -> guard -> guarded step).
 *
 * rfn_grad_sumsq_f32: sumsq[0] = sum of g^2 over the tensors whose flags bit 0 is clear, sumsq[1] = over those with it
 * set.  `partials` is a caller-provided workspace of n_chunks floats.  Two launches: one workgroup per chunk stores that
 * chunk's partial (<= 32 serial fp32 adds per lane, then a fixed tree), one workgroup adds the partials in a fixed order
 * in double and rounds once.  No float atomics: equal inputs give bit-identical results on every run and every rank.
 *
 * rfn_grad_guard_f32 (one tiny launch): with s = sumsq[0] + sumsq[1] in double,
 *   stats[0] = norm  = sqrt(s), rounded to float;
 *   stats[1] = scale = min(1, max_norm / (norm + 1e-6)) in double, rounded once (torch's clip_grad_norm_); 1 when
 *              max_norm <= 0;
 *   stats[2] = 1.0 if skip_nonfinite != 0 and the norm is not finite, else 0.0; then *skipped is incremented.
 * A sum of squares that overflows fp32 COUNTS AS NON-FINITE, although a wider format could still hold it: the partial
 * sums are fp32, and s itself is tested after rounding to float.
 *
 * rfn_adam_step_guarded_f32: rfn_adam_step_f32 with three differences.  stats[2] != 0: nothing is written (p, m, v keep
 * their bits).  The gradient used is stats[1] * g, applied before weight decay (clipping precedes the optimizer); g is
 * never written.  A tensor's step count is t - step_offset - *skipped, so bias correction does not advance over skipped
 * steps.  With stats[1] == 1.0f and *skipped == 0 the update is bit-identical to rfn_adam_step_f32.  `skipped` is only
 * read here. */
int rfn_grad_sumsq_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, float* partials, float* sumsq,
                       rfn_stream_t stream);
int rfn_grad_guard_f32(const float* sumsq, double max_norm, int skip_nonfinite, float* stats, long long* skipped,
                       rfn_stream_t stream);
int rfn_adam_step_guarded_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1,
                              double beta2, double eps, double weight_decay, int t, const float* stats,
                              long long* skipped, rfn_stream_t stream);

/* ---- Polyak average (EMA) of the weights inside the Adam launch.  rfn_adam_ema_step_f32 / rfn_adam_ema_step_guarded_f32
 * are rfn_adam_step_f32 / rfn_adam_step_guarded_f32 plus `ema_decay` d in [0, 1) and `ema`, a DEVICE array of one device
 * pointer per table entry (ema[i] has table[i].n floats).  With n = that tensor's count of APPLIED steps (the s of the bias
 * corrections: t - step_offset, minus *skipped in the guarded kernel), after the update has produced p_new:
 *   d_n = min(d, (1 + n) / (10 + n))   in double;   w = (float)(1 - d_n);   ema <- fmaf(w, p_new - ema, ema)   in fp32.
 * p, m, v receive the bits the kernel without the average gives on the same inputs.  The 16-byte path needs ema[i]
 * aligned like p, g, m, v; otherwise the chunk takes the scalar loop (same arithmetic).  A step the guard skips writes
 * nothing to ema.  ema_decay outside [0, 1) or a NULL `ema` is refused (-3 / -1) and nothing is launched.
 *
 * rfn_param_swap_f32: one launch over the same table and chunk list that exchanges p and ema element-wise (bit-exact
 * moves: two launches are the identity).  g, m, v are not touched. */
int rfn_adam_ema_step_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1,
                          double beta2, double eps, double weight_decay, int t, double ema_decay, float* const* ema,
                          rfn_stream_t stream);
int rfn_adam_ema_step_guarded_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, int t, const float* stats,
                                  long long* skipped, double ema_decay, float* const* ema, rfn_stream_t stream);
int rfn_param_swap_f32(const rfn_adam_entry* table, const int* chunks, int n_chunks, float* const* ema,
                       rfn_stream_t stream);

/* ---- video-prediction quality of uint8 frames  (evaluation_metrics/error_metrics.py:154-171, Evaluator.eval_seq: skimage
 * 0.17.2 `structural_similarity` / `peak_signal_noise_ratio` per channel, with their defaults on uint8: 7x7 uniform window,
 * data_range 255, K1 = 0.01, K2 = 0.03, sample covariance (x 49/48), S map averaged over the interior (H-6) x (W-6)).
 * a, b: uint8 NCHW frames (frame strides a_ns / b_ns in elements, i.e. bytes); per frame n (float32 [N] outputs):
 *   mse[n]  = sum of squared differences / (C*H*W),
 *   psnr[n] = mean over channels of 10 log10(255^2 / mean((a-b)^2)), +inf when a channel is identical,
 *   ssim[n] = mean over channels of the single-channel SSIM.
 * Window sums and (co)variances are exact integers, the S formula runs in fp64, reductions in a fixed order: results
 * are bit-reproducible.  H < 7 or W < 7 is an argument error (skimage: "win_size exceeds image extent"). */
int rfn_frame_quality_u8(const void* a, long a_ns, const void* b, long b_ns, float* mse, float* psnr, float* ssim,
                         int N, int C, int H, int W, rfn_stream_t stream);

/* ---- Stochastic Moving MNIST rendered on the device  (data_generators/stochasticMovingMnist.py:48-127,
 * MovingMNIST.__getitem__ as RFN/trainer.py:112-131 calls it: normalize=False; digit_size 28, for which the Resize(28)
 * of :33-37 is the identity).  digits: uint8 [N, 28, 28] device table.  Writes out: fp32 [B, T, C, S, S] in [0, 1]
 * (16-byte aligned for the vector stores; any 4-byte alignment works), sequence b of the launch having the id
 * first_id + b; traj (nullable): int64 [B, num_digits, T, 3] of (digit index, y, x) per digit and frame.  Every random
 * draw is addressed: Philox4x64-10 with key (seed, split) and counter (draw number, retry, sequence id, digit), bounded
 * by Lemire's multiply-shift with rejection (csrc/moving_mnist.hip states the scheme); the walk, its draw order and the
 * float32 pixel pipeline are the reference's.  deterministic != 0: a wall bounce negates the velocity component.
 * Limits: 28 < S <= 4096, 1 <= num_digits <= 8, step_length >= 1, seed, split, first_id >= 0.  One launch. */
int rfn_moving_mnist_render_f32(const void* digits, int N, float* out, long long* traj, int B, int T, int C, int S,
                                int num_digits, int step_length, int deterministic, long seed, long split,
                                long first_id, rfn_stream_t stream);

/* The synchronized variant (MovingMNIST_synchronized, stochasticMovingMnist.py:131-248): all sequences share one
 * trajectory per digit, only the digit identities differ.  Walk of digit n: idx = randint(N), sx, sy = randint(S - 28),
 * dx = dy = 3 (a constant whatever step_length is, as the reference has it), then per frame the y-bounce and x-bounce
 * of the entry above with step_length and deterministic.  idx is draw 0 at the counter (0, retry, sequence id, n) of
 * the entry above; every other draw uses the shared counter (j, retry, 2^64 - 1, n), j = 1 for sx, 2 for sy, 3, 4, ...
 * for the bounce redraws in walk order (sequence ids are non-negative, so no id collides with it).  out, traj and the
 * limits are those of the entry above.  hit_addr: the device address of hit, int32 [B, T] (4-byte aligned), or 0 for
 * none (passed as an integer like the byte outputs' out_addr); hit[b, t] is the largest n + 1 over the digits that
 * either bounce branch clamped on frame t (the reference's hit_boundary: the last digit wins), 0 if none; every row
 * holds the same values.  No atomics, every output element is written exactly once.  One launch. */
int rfn_moving_mnist_sync_render_f32(const void* digits, int N, float* out, long long* traj, long hit_addr, int B, int T,
                                     int C, int S, int num_digits, int step_length, int deterministic, long seed,
                                     long split, long first_id, rfn_stream_t stream);

/* ---- addressed normal noise  (the draws of RFN.predict_draws and of the Evaluator's batched best-of-N; DESIGN.md
 * section 16).  One launch fills up to 8 tensors ("slots") of shape [rows, numel_j], fp32 contiguous, with N(0,1) values.
 * Each value depends only on its address, not on the launch geometry.
 * Row i of a launch stands for (draw, sequence): draw = first_draw + i / B, seq = first_seq + i % B (draw-major:
 * row i = r_local * B + b).
 * Block q of slot j at step t is Philox4x64-10(key = (seed, (t << 32) | j), counter = (q, 0, seq, draw)).  It has four
 * 64-bit words w0..w3 (the round function and constants of csrc/moving_mnist.hip; csrc/philox.h).
 * Word w_i of block q gives elements 8q + 2i and 8q + 2i + 1 of the row (flattened C*H*W):
 *   a = w >> 32, b = w & 0xffffffff
 *   u1 = ((a >> 8) + 1) * 2^-24, in (0, 1]
 *   u2 = (b >> 8) * 2^-24, in [0, 1)
 *   rad = sqrtf(-2 * logf(u1))
 *   the two values are rad * cospif(2 * u2) and rad * sinpif(2 * u2),
 * with the accurate fp32 functions, not fast-math intrinsics; 2 * u2 is exact, so no rounded 2 pi enters;
 * |value| <= sqrt(48 ln 2) ~ 5.77.
 * outs, numels: HOST arrays of n_slots device pointers and row lengths, 1 <= n_slots <= 8; slot j is the array position;
 * numels[j] == 0 skips slot j (its pointer is not read).  rows is a multiple of B >= 1; seed, first_seq, first_draw and
 * step are >= 0 (step and j are 32-bit words of the key).  Two 16-byte stores per lane where numels[j] % 8 == 0 and
 * outs[j] is 16-byte aligned, single stores otherwise (outs[j] must be 4-byte aligned).  No atomics, no LDS.  One launch
 * (none when nothing is to be written). */
int rfn_keyed_normal_f32(float* const* outs, const int* numels, int n_slots, int rows, int B, long seed, int step,
                         long first_seq, long first_draw, rfn_stream_t stream);
/* the same values `tiles` >= 1 times (common random numbers for a temperature sweep): every tensor
 * is [tiles * rows, numel_j] and row k * rows + i holds exactly what row i holds above, for every tile k.  Still one
 * launch of the untiled grid: a lane computes its eight values once and stores them `tiles` times.  tiles * rows must
 * fit an int.  tiles == 1 is rfn_keyed_normal_f32. */
int rfn_keyed_normal_tiled_f32(float* const* outs, const int* numels, int n_slots, int rows, int B, int tiles, long seed,
                               int step, long first_seq, long first_draw, rfn_stream_t stream);

/* ---- RFN's importance-weighted bound, csrc/iw_bound.hip  (RFN.iw_log_weights; DESIGN.md section 24 is the contract).
 * rfn_latent_iw_f32: one latent step of `rows` chains.  enc, pri = [rows, 2*ZHW] outputs of the encoder / prior parameter
 * convs in rfn_latent_step_fwd_f32's layout (loc half | raw scale half), eps_q [rows, ZHW]; with ps = softplus(pri_raw),
 * es = softplus(enc_raw) (nothing added), pm = pri_loc, em = enc_loc (+ pm when res_q):
 *   zxt = em + es*eps_q                       [rows, ZHW], bit for bit rfn_latent_step_fwd_f32's zxt of the same inputs;
 *   logr[row] = sum_j  -((zxt - pm)/ps)^2 / 2 - log ps + eps_q^2 / 2 + log es           [rows]
 * i.e. log N(zxt; pm, ps) - log N(zxt; em, es) summed over the row (the 2 pi terms cancel).  An element's term is
 * evaluated in fp64 on the fp32 values zxt, pm, ps, es, eps_q and rounded to fp32 once (its parts nearly cancel where
 * posterior and prior are close); the sum is fp32.  Forward only.
 * One wavefront per row, four rows per workgroup; lane l adds the terms of elements l, l + 64, ... in index order and the
 * 64 lane sums are combined by a fixed xor butterfly (32, 16, ..., 1): no atomics, no LDS memory, a row's bits depend on
 * that row alone (not on rows or the grid).  Any rows >= 1, ZHW >= 1; -1 (nothing launched) for smaller sizes or a NULL
 * pointer.  One launch, no allocation: capturable. */
int rfn_latent_iw_f32(const float* enc, const float* pri, const float* eps_q, float* zxt, float* logr, int rows, int ZHW,
                      int res_q, rfn_stream_t stream);
/* rfn_keyed_uniform_f32: addressed uniforms in [0, scale), the dequantisation noise of all steps of a pass in one
 * launch.  out [n_steps, rows, numel] fp32 contiguous; row i of every step-block stands for draw first_draw + i / B of
 * sequence first_seq + i % B (draw-major, as rfn_keyed_normal_f32), step-block s for step first_step + s.
 * Block q of a row is Philox4x64-10(key = (seed, (step << 32) | slot), counter = (q, 0, seq, draw)), words w0..w3
 * (csrc/philox.h).  Word w_i gives element 8q + 2i from its high half and element 8q + 2i + 1 from its low half:
 *   value = (half >> 8) * 2^-24 * scale
 * The first product is exact and the second is rounded once: every value lies in [0, scale).  A value depends only on
 * (seed, step, slot, sequence, draw, element): not on rows, B, n_steps, the grid or the split into calls.
 * slot in [8, 2^31): rfn_keyed_normal_f32 owns slots 0..7 of this key space, rfn_mol_sample_keyed uses 16 and 17 with
 * another counter; RFN.iw_log_weights uses 24.  rows is a multiple of B >= 1; seed, first_seq, first_draw, first_step
 * are >= 0 and first_step + n_steps <= 2^31; scale is finite and > 0.  Two 16-byte stores per lane where numel % 8 == 0
 * and out is 16-byte aligned, single stores otherwise (out must be 4-byte aligned).  No atomics, no LDS.  One launch (none
 * when nothing is to be written); a failed check launches nothing. */
int rfn_keyed_uniform_f32(float* out, int n_steps, int rows, int B, int numel, float scale, long seed, int first_step,
                          int slot, long first_seq, long first_draw, rfn_stream_t stream);

/* ---- clips of a device-resident frame store as float32 batches  (the per-item work of the file-backed datasets,
 * data_generators/bair_push.py:66-109 and data_generators/kth.py:34-65, and the DataLoader collation of
 * RFN/trainer.py:132-161, for a whole batch in one launch).  store: uint8 [n_frames, H, W, Cs] device tensor,
 * channel-interleaved as an image decoder leaves it, Cs in {1, 3}; first: int64 [B] device tensor, the store index of
 * each clip's first frame.  Writes out: fp32 [B, T, C, H, W],
 *   out[b,t,c,y,x] = float32(store[first[b]+t, y, x, c']) / float32(255)   (the correctly rounded float32 quotient),
 * c' = c when C == Cs, c' = 0 when Cs == 1 (C in {1, 3} copies); any other (C, Cs) is an argument error.  A clip with
 * first[b] < 0 or first[b] + T > n_frames reads nothing: all its T frames are NaN.  16-byte loads and float4 stores
 * when H*W is a multiple of 4, H*W*Cs a multiple of 16 and both bases are 16-byte aligned; single pixels otherwise.
 * B == 0 returns 0 without a launch.  One launch. */
int rfn_clip_gather_u8_f32(const void* store, long n_frames, const void* first, float* out, int B, int T, int C, int Cs,
                           int H, int W, rfn_stream_t stream);
/* rfn_clip_gather_aug_u8_f32: the same gather with a temporal stride and two per-clip augmentations (csrc/clip_gather.hip;
 * data_generators/clip_folder.py).  store, n_frames, first, out, B, T, C, Cs, H, W as above;
 * step >= 1: store frames between two frames of a clip; flags: int32 [B] device tensor or NULL (all 0), bit 0 mirrors x,
 * bit 1 reverses time, other bits are ignored.
 *   out[b,t,c,y,x] = lut[ store[first[b] + tt*step, y, xx, c'] ],   tt = bit1 ? T-1-t : t,   xx = bit0 ? W-1-x : x
 * with the same correctly rounded k/255 table and the same channel rule c'.  A clip with first[b] < 0 or
 * first[b] + (T-1)*step + 1 > n_frames reads nothing: all its T frames are NaN.  With flags == NULL and step == 1 the
 * output is rfn_clip_gather_u8_f32's bit for bit.  16-byte loads and float4 stores under rfn_clip_gather_u8_f32's
 * conditions; a mirrored clip keeps them where W % 4 == 0 (the four pixels of a group are reversed in registers and
 * stored at the mirrored group of their row) and goes pixel by pixel at any other width.  No atomics, no scratch.
 * Returns -1 for sizes or a step below their minimum, -2 for the channel rule, -3 / -4 for a frame or a batch beyond one
 * launch, -5 for a NULL store, first or out, -6 for flags that are not 4-byte aligned; nothing is launched then.  B == 0
 * returns 0 without a launch.  One launch, no allocation: capturable. */
int rfn_clip_gather_aug_u8_f32(const void* store, long n_frames, const void* first, const void* flags, float* out, int B,
                               int T, int C, int Cs, int H, int W, int step, rfn_stream_t stream);

/* ---- frames of any size and channel count into a frame store's geometry  (csrc/frame_resize.hip; the ingest step of
 * data_generators/clip_folder.py).  src: uint8 [F, Hs, Ws, Cs] device tensor, channel-interleaved,
 * of any byte alignment; dst_addr: the device address of the uint8 output [F, H, W, Cd], of any byte alignment (the
 * header has no mutable byte pointer type); Cs, Cd in {1, 3}; (y0, x0, Hc, Wc): the crop window, which must lie
 * inside the source frame.  Exact integer area mean, rounded half up: output row y covers [y*Hc, (y+1)*Hc) on a grid
 * where window row i covers [i*H, (i+1)*H), so
 *   wy(i) = min((y+1)*Hc, (i+1)*H) - max(y*Hc, i*H)   for i = floor(y*Hc/H) .. ceil((y+1)*Hc/H) - 1
 * (every wy(i) > 0, their sum is Hc), wx(j) alike with W and Wc, and per stored channel
 *   v = (sum_i sum_j wy(i) * wx(j) * src[f, y0+i, x0+j, c] + (Hc*Wc)/2) / (Hc*Wc)            (integer division)
 * accumulated in 64 bits.  Equal sizes give the identity, a constant frame stays constant, enlarging is the same
 * formula.  Channels, on the rounded bytes: Cs == Cd copies; 3 -> 1 is (19595 R + 38470 G + 7471 B + 32768) >> 16;
 * 1 -> 3 is three copies.  Every output byte is written exactly once; nothing is read outside the windows.
 * One workgroup per (frame, band of output rows); the source rows under the band pass through LDS in pieces of at most
 * 2 KiB of a row, with 16-byte loads when src is 16-byte aligned and Ws*Cs is a multiple of 16, single bytes otherwise.
 * No atomics, no scratch.  Returns -1 for F < 0 or a side outside [1, 32768], -2 for channel counts other than 1 and 3,
 * -3 for an empty window or one that leaves the frame, -4 for more than 2^31 - 1 workgroups, -5 for a NULL src or a
 * dst_addr of 0; nothing is launched then.  F == 0 returns 0 without a launch.  One launch, no allocation: capturable. */
int rfn_frames_resize_u8(const void* src, long dst_addr, long F, int Hs, int Ws, int Cs, int H, int W, int Cd, int y0, int x0,
                         int Hc, int Wc, rfn_stream_t stream);

/* ---- a sheet of frames as 8-bit RGB pixels  (the subplot grids of plotter(), RFN/trainer.py:325-417, and of
 * Evaluator.plot_samples, evaluation_metrics/error_metrics.py:128-152, as pixels only: no text, axes or titles).
 * R rows x N columns of H x W cells with `gutter` pixels of the grey level `bg` between the cells and around the sheet:
 *   Hs = R*H + (R+1)*gutter,  Ws = N*W + (N+1)*gutter,  cell (r, i) at (gutter + r*(H+gutter), gutter + i*(W+gutter)).
 * rows_table: HOST array of R rfn_sheet_row, copied into the launch (R <= RFN_SHEET_MAX_ROWS): the frame of cell (r, i)
 * is the dense [C, H, W] block at ptr + i*step (in elements; rows may be views such as image[0, i] of [B,T,C,H,W] or
 * samples[i, 0] of [T,B,C,H,W]) for i < count, 0 <= count <= N; cells i >= count are background.  kind 0: fp32 in
 * model space, turned into a byte as Solver.preprocess(x, reverse=True) does (RFN/trainer.py:165-188):
 *   v = x + 0.5 if range_half else x;  v = v * 2^n_bits;  q = floor(v) * (256 / 2^n_bits);  byte = clamp(q, 0, 255),
 * NaN -> 0, every operation rounded to fp32 on its own (all factors are powers of two: bit-equal to torch).  kind 1:
 * uint8, copied.  C in {1, 3}; C == 1 writes the value to R, G and B; any other C is an argument error.
 * out_addr: the device address of the uint8 output, of any byte alignment (the header has no mutable byte pointer type):
 * lead 0: [Hs, Ws, 3];  lead 1: [Hs, 1 + 3*Ws] with byte 0 of every line 0, the PNG filter type "None", i.e. the raw
 * stream of a PNG before deflate.  Every output byte is written exactly once (nothing needs zeroing), with dword stores
 * on the 4-byte-aligned part of each line and byte stores at its ragged ends; no atomics; nothing is read outside the
 * listed frames.  1 <= n_bits <= 8, 0 <= bg <= 255, gutter >= 0.  One launch. */
#define RFN_SHEET_MAX_ROWS 32
typedef struct rfn_sheet_row {
    const void* ptr;
    long step;
    int kind;
    int count;
} rfn_sheet_row;
int rfn_sheet_max_rows(void);
int rfn_sheet_compose_u8(const void* rows_table, int R, int N, int C, int H, int W, int gutter, int bg, int n_bits,
                         int range_half, int lead, long out_addr, rfn_stream_t stream);

/* ---- a line chart as 8-bit RGB pixels from a display list  (the matplotlib figures of Evaluator.test_temp_values and
 * Evaluator.plot_eval_values, evaluation_metrics/error_metrics.py:600-809 and :812-1003: lines, fill_between bands,
 * markers, error bars, axvline, grid, axes and text; DESIGN.md section 25 is the pixel contract, integer throughout).
 * table: DEVICE array of n records of 12 int32 {type, rgba, p0..p9}, 16-byte aligned, painted in list order;
 *   rgba = r | g<<8 | b<<16 | alpha<<24; geometry in 1/16 pixel, x right, y down, every coordinate in [-4096, 36864],
 *   every capsule half-width in [0, 4096] (all products fit 64 bits).  A sample s = (sx, sy) is inside
 *   0 BOX        p0..p3 = x0, y0, x1, y1: x0 <= sx < x1, y0 <= sy < y1; p4, p5 = dash on, off (>= 0): when on + off > 0
 *                also ((t - t0) mod (on + off)) < on, t the sample's coordinate on the long axis (x if x1 - x0 >=
 *                y1 - y0, else y), t0 the box's start on it;
 *   1 CAPSULE    p0..p4 = ax, ay, bx, by, hw; d = b - a, p = s - a: p.d <= 0: |p|^2 <= hw^2; p.d >= |d|^2:
 *                |s - b|^2 <= hw^2; else (d x p)^2 <= hw^2 |d|^2  (a == b: a disc);
 *   2 TRAPEZOID  p0..p5 = x0, x1, lo0, lo1, hi0, hi1: x0 <= sx < x1, (sy - lo0)(x1 - x0) >= (lo1 - lo0)(sx - x0),
 *                (sy - hi0)(x1 - x0) < (hi1 - hi0)(sx - x0);
 *   3 TRIANGLE   p0..p5 = x0, y0, x1, y1, x2, y2: e_i = (x_j - x_i)(sy - y_i) - (y_j - y_i)(sx - x_i) over the edges
 *                (0,1), (1,2), (2,0): all e_i >= 0 or all e_i <= 0; nothing when the area is zero, i.e. when
 *                (x1 - x0)(y2 - y0) == (y1 - y0)(x2 - x0);
 *   4 GLYPH      p0, p1 = top-left x, y, p2 = ASCII code 32..126, p3 = scale k in 1..128 (pixels per dot), p4 = 0
 *                upright, 1 rotated 90 degrees counter-clockwise; u = sx - x, v = sy - y, q = 16 k; upright: 0 <= u < 5q,
 *                0 <= v < 7q and dot (column floor(u/q), row floor(v/q)) of the built-in 5x7 font is set; rotated:
 *                0 <= u < 7q, 0 <= v < 5q and dot (column 4 - floor(v/q), row floor(u/q)) is set.
 *   Any other record paints nothing.  Pixel (px, py) has the 16 samples (16 px + i, 16 py + j), i, j in {2, 6, 10, 14};
 *   per record, with c = samples inside and w = alpha * c: dst = (dst (4080 - w) + src w + 2040) / 4080 per channel in
 *   integer division, from the background bg = r | g<<8 | b<<16.
 * H, W: the canvas, 1..2048 each.  out_addr: the device address of the uint8 output, any byte alignment: lead 0:
 * [H, W, 3]; lead 1: [H, 1 + 3 W] with byte 0 of every line 0 (the raw stream of a PNG, as rfn_sheet_compose_u8).  Every
 * output byte is written exactly once, nothing outside it whatever the table holds; no atomics; the result does not
 * depend on rfn_chart_chunk(), the records one workgroup culls against its 16 x 16 tile at a time.  One launch.
 * rfn_chart_font (host only): out[5 ch + c] = column c (left to right) of character 32 + ch, bit r = the dot of row r
 * from the top; 475 values. */
int rfn_chart_chunk(void);
int rfn_chart_font(long long* out);
int rfn_chart_render_u8(const int* table, int n, int H, int W, int bg, int lead, long out_addr, rfn_stream_t stream);

/* ---- an animation of prediction draws as 8-bit RGB pixels, csrc/clip_compose.hip  (the moving counterpart of
 * rfn_sheet_compose_u8: ground truth, draws, their mean and their spread side by side, each cell inside a coloured ring
 * as the reference's figures frame their subplots; DESIGN.md section 28 is the pixel contract).  One launch writes all T
 * frames.  Every frame is a grid of R x N cells of Hc x Wc = (zoom*H + 2*border) x (zoom*W + 2*border) pixels with
 * `gutter` pixels of the grey level `bg` between the cells and around the grid:
 *   Hs = R*Hc + (R+1)*gutter,  Ws = N*Wc + (N+1)*gutter,  cell (r, i) at (gutter + r*(Hc+gutter), gutter + i*(Wc+gutter)).
 * cells: DEVICE array of R*N records of eight int64 words, 8-byte aligned, cell (r, i) at index r*N + i (a device table,
 * as the chart's: the cell count is not bounded by the launch's arguments); its contents are the caller's responsibility:
 *   w0  byte address of member 0, frame 0 (4-byte aligned for kind 0; 0 for an empty cell)
 *   w1  elements between consecutive frames          w2  elements between consecutive group members
 *   w3  count, the frames available (0: an empty cell)
 *   w4  group size G, 1..RFN_CLIP_MAX_GROUP
 *   w5  kind | mode << 8 | gain << 16: kind 0 fp32 in model space, 1 uint8; mode 0 FRAME, 1 MEAN, 2 SPREAD;
 *       gain 1..RFN_CLIP_MAX_GAIN
 *   w6  switch_at                                     w7  rgb_before | rgb_after << 32, a colour being r | g<<8 | b<<16
 * Frames are dense [C, H, W] blocks, C in {1, 3}; C == 1 goes to R, G and B.  Pixel rules of frame t, integer after the
 * byte conversion: b_g = the byte of member g at source pixel (c, y, x) of frame f = min(t, count - 1), made as
 * rfn_sheet_compose_u8 makes it (kind 0: Solver.preprocess(x, reverse=True) with n_bits / range_half, NaN -> 0; kind 1:
 * a copy);
 *   FRAME   b_0
 *   MEAN    (sum_g b_g + G/2) / G
 *   SPREAD  min(255, isqrt(gain^2 (G sum_g b_g^2 - (sum_g b_g)^2)) / G): gain times the population standard deviation
 *           of the bytes, rounded down; isqrt is the exact integer square root (the radicand has at most 44 bits)
 * with floor divisions and sums in member order.  Zoom is nearest: interior pixel (yy, xx) of a cell shows source pixel
 * (yy / zoom, xx / zoom).  The ring of `border` pixels around the interior has the colour rgb_before for t < switch_at,
 * else rgb_after.  An empty cell is all bg, ring included.
 * out_addr: the device address of the uint8 output, of any byte alignment: lead 0: [T, Hs, Ws, 3];  lead 1:
 * [T, Hs, 1 + 3*Ws] with byte 0 of every line 0, i.e. T raw PNG streams.  Every output byte is written exactly once
 * (dword stores on the aligned part of each line, byte stores at its ragged ends), nothing outside it; only listed
 * frames are read; no atomics, no LDS, no scratch.  One launch, no allocation: capturable.
 * Returns -1 unless R, N, T, H, W >= 1; -2 unless C in {1, 3}; -3 unless 1 <= zoom <= 16, 0 <= border <= 64, gutter >= 0
 * and 0 <= bg <= 255; -4 unless 1 <= n_bits <= 8 and lead in {0, 1}; -5 unless 3*Ws + lead <= 2^31 - 1 and T*Hs <=
 * 2^31 - 1; -6 for a NULL table or an out_addr of 0; nothing is launched then.  The two limits are read by the binding
 * through the host-only queries below (they are written in parentheses, like RFN_LINEXT_MAX_FRAMES). */
#define RFN_CLIP_MAX_GROUP (1024)
#define RFN_CLIP_MAX_GAIN (16)
int rfn_clip_max_group(void);
int rfn_clip_max_gain(void);
int rfn_clip_compose_u8(const void* cells, int R, int N, int T, int C, int H, int W, int zoom, int border, int gutter,
                        int bg, int n_bits, int range_half, int lead, long out_addr, rfn_stream_t stream);

/* ---- LPIPS with the AlexNet trunk over a batch of uint8 frames  (evaluation_metrics/error_metrics.py:72, :173-187:
 * lpips.LPIPS(net='alex') of `lpips` 0.1.3, version 0.1, lpips=True, spatial=False, eval mode; one call per frame there).
 * Frame [C, H, W] uint8, C in {1, 3} (one channel stands for all three): x = p/255*2 - 1, then (x - shift[c]) / scale[c]
 * with shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  Five taps, each after a ReLU, all convolutions with
 * bias and zero padding in the scaled domain: conv 3->64 11x11 stride 4 pad 2 | maxpool 3x3 stride 2, conv 64->192 5x5
 * pad 2 | maxpool 3x3 stride 2, conv 192->384 3x3 pad 1 | conv 384->256 3x3 pad 1 | conv 256->256 3x3 pad 1.  Head: per
 * tap l and pixel n(f) = f / (sqrt(sum_c f_c^2) + 1e-10), d_l = mean over pixels of sum_c lin_l[c] (n(fa)_c - n(fb)_c)^2,
 * d = d_1 + ... + d_5 in tap order.  H, W >= 31 (the second pool needs a 3x3 map); smaller is an argument error.
 *
 * rfn_lpips_alex_sizes (host only, no GPU needed): out[0..9] = (rows, columns) of the five taps, out[10] = floats per
 *   frame of the feature pack (the taps one after the other, each [rows*columns][channels], channels 64, 192, 384, 256,
 *   256), out[11] = workspace floats per frame.
 * rfn_lpips_alex_weight_layout (host only): the packed trunk weights are one float buffer; out[l] = offset of
 *   convolution l's weights, [Kpad_l][Cout_l] with k = (ky*ks + kx)*Cin + ci and zero rows from Cin*ks*ks up to Kpad_l;
 *   out[5 + l] = offset of its Cout_l biases; out[10 + l] = Kpad_l; out[15] = floats in all.
 * rfn_lpips_alex_features_u8: the trunk.  frames: uint8 NCHW, frame stride in bytes; feats_out: [N][out[10]];
 *   workspace: at least N * out[11] floats, free again when the call's work is done.  Convolutions on
 *   v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fma chain per value): a frame's features do not depend on
 *   its index, on N or on how a batch is split into calls, and C == 1 gives the bits of three identical channels.
 *   Seven launches.
 * rfn_lpips_alex_distance: the head.  feats_a, feats_b: [N][out[10]]; lin: the 1152 lin weights in tap order;
 *   per_layer_out: [N][5] = d_l; out: [N] = d.  Fixed reduction order, no atomics: bit-reproducible, exactly 0 on equal
 *   features and the same bits for (a, b) and (b, a).  One launch. */
int rfn_lpips_alex_sizes(int H, int W, long long* out);
int rfn_lpips_alex_weight_layout(long long* out);
int rfn_lpips_alex_features_u8(const void* frames, long frame_stride, int N, int C, int H, int W, const float* wpack,
                               long wpack_floats, float* feats_out, float* workspace, long workspace_floats,
                               rfn_stream_t stream);
int rfn_lpips_alex_distance(const float* feats_a, const float* feats_b, const float* lin, int N, int H, int W,
                            float* per_layer_out, float* out, rfn_stream_t stream);

/* ---- Inflated-3D Inception trunk (I3D, Kinetics-400, RGB stream) for the Frechet Video Distance (evaluation_metrics/
 * FVD.py, FVD_score.py, error_metrics.py:1006-1063; DESIGN.md section 14 is the definition).  rfn_hip/i3d.py holds the
 * layer table and drives these kernels layer by layer.  Activations are channels-last float32 [N, T, H, W, C]; every
 * convolution and pool pads as TF "SAME": out = ceil(in / s), pad_total = max((out - 1) s + k - in, 0), pad_before =
 * pad_total / 2, the rest after.
 *
 * rfn_i3d_same (host only): out[0] = output extent, out[1] = pad before, of one axis.
 * rfn_i3d_conv_pack_dims (host only): out[0] = Kpad (Cin k^3 rounded up to the k chunk), out[1] = Coutpad (Cout rounded up
 *   to the column tile) of a packed convolution [Kpad][Coutpad], k = ((kt k + ky) k + kx) Cin + ci, zero rows and columns
 *   past K and Cout; the bias has Coutpad entries.
 * rfn_i3d_conv3d_f32: cubic convolution (k in {1, 3, 7}, stride 1 or 2 on every axis) + bias + optional ReLU as an implicit
 *   GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fma chain per value: a value does not depend on
 *   N or on the position of its video in the call).  in: dense [N, T, H, W, Cin]; out: rows of out_pitch floats, one per
 *   output position, the Cout values written at out_coff (everything else in the row is left alone).
 * rfn_i3d_maxpool3d_f32: SAME max pool, window kt x khw x khw, stride st x shw x shw, dense in and out; cells outside the
 *   map are ignored, not read as zero.
 * rfn_i3d_resize_u8: uint8 frames [NF][C][H][W] (C in {1, 3}, one channel standing for three; frame stride in bytes) to
 *   float [NF][224][224][3] with TF1's resize_bilinear (align_corners=False, no half-pixel centres), then 2 v / 255 - 1.
 * rfn_i3d_head_f32: in [N][Tp][P][C] -> out [N][Cout]: average over windows of 2 time steps x all P cells (stride 1,
 *   VALID), logits bias + avg w from a packed [C][Coutpad] convolution, mean over the Tp - 1 windows; fixed order.
 * The *_floats arguments are the sizes of the buffers; the entry points refuse a call that would leave them.
 * No atomics anywhere. */
int rfn_i3d_same(int in, int k, int s, long long* out);
int rfn_i3d_conv_pack_dims(int Cin, int Cout, int k, long long* out);
int rfn_i3d_conv3d_f32(const float* in, long in_floats, int N, int T, int H, int W, int Cin, const float* wpack,
                       long wpack_floats, const float* bias, int Cout, int k, int stride, int relu, float* out,
                       long out_floats, int out_coff, int out_pitch, rfn_stream_t stream);
int rfn_i3d_maxpool3d_f32(const float* in, long in_floats, int N, int T, int H, int W, int C, int kt, int khw, int st,
                          int shw, float* out, long out_floats, rfn_stream_t stream);
int rfn_i3d_resize_u8(const void* frames, long frame_stride, int NF, int C, int H, int W, float* out, long out_floats,
                      rfn_stream_t stream);
int rfn_i3d_head_f32(const float* in, long in_floats, int N, int Tp, int P, int C, const float* wpack, long wpack_floats,
                     const float* bias, int Cout, float* out, rfn_stream_t stream);

/* ---- the linear-extrapolation baseline, csrc/linear_extrap.hip  (averagemodel/averagemodel.py, SimpleLinearModel;
 * DESIGN.md section 26 is the contract).  x: float32 [B, T, C, H, W] whose frames are dense blocks of CHW = C*H*W
 * floats, seq_stride / frame_stride in elements; the window is frames start .. start+n-1 of every sequence, read in
 * place.  Features of one pixel's window x_0 .. x_{n-1}, in this order: x_f for f = 0 .. n-1, then for k = 0 .. n-2 and
 * inside that j = 0 .. n-k-2 the difference x_j - x_{j+k+1} (get_lagged_differences, :65-71); F = n (n + 1) / 2,
 * 1 <= n <= RFN_LINEXT_MAX_FRAMES.  w: F floats, bias: 1 float;  pred = bias + sum_f w[f] feat_f as one fma chain in
 * feature order, the differences formed in registers (never collapsed into per-frame weights).  16-byte loads and
 * stores when CHW and both strides are multiples of 4 and the bases are 16-byte aligned, single floats otherwise.
 *
 * rfn_linext_train_f32: target = frame start+n (start + n + 1 <= T), r = pred - target;
 *   out[0] = mean r^2 over B*CHW,  out[1 + f] = mean 2 r feat_f  (= dL/dW[f]),  out[F + 1] = mean 2 r  (= dL/dbias).
 *   Stage 1 (grid sized to the device, at most rfn_linext_max_blocks() workgroups and partial_floats / (F + 2)) writes
 *   per-workgroup fp32 sums [blocks, F+2] to `partials`; stage 2, one workgroup, adds the rows in row order in fp64
 *   and rounds once.  Two launches, no allocation.
 * rfn_linext_rollout_f32: out [B, P, C, H, W] dense; frame t is pred of the window, which then drops its oldest frame
 *   and takes the prediction (no clamping); a thread keeps its pixels' window in registers and writes all P frames.
 *   start + n <= T, P >= 1; P = 1 is get_prediction.  One launch.
 * rfn_gauss_quality_f32: pred, truth float32 [N, C, H, W] dense, read once as clamp(v * scale, lo, hi); per image
 *   mse[n] = mean over C*H*W of the squared difference, and ssim[n] = pytorch_msssim.ssim(X, Y, data_range=255) of
 *   that image: window g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1, applied separably per
 *   channel without padding ((H-10) x (W-10) outputs); mu1 = g*X, mu2 = g*Y, s1 = g*(X X) - mu1^2, s2 = g*(Y Y) - mu2^2,
 *   s12 = g*(X Y) - mu1 mu2, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 *   map = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) ((2 s12 + C2) / (s1 + s2 + C2)); mean of map, then over channels.
 *   The five row sums of a chunk of rows are fp32 fma chains formed in LDS from one load of X and Y; the column pass
 *   and the formula run in fp64.  RFN_GAUSS_QUALITY_MIN_SIDE <= H, W <= RFN_GAUSS_QUALITY_MAX_SIDE.  One workgroup per image, one launch.
 * All three: no atomics, fixed reduction orders (bit-identical run to run on one device); a bad size returns -1, a
 * NULL pointer -2, and nothing is launched.  The three limits are read by the binding through the host-only queries
 * below, like rfn_sheet_max_rows() (they are written in parentheses: the binding mirrors plain-integer defines only). */
#define RFN_LINEXT_MAX_FRAMES (10)
#define RFN_GAUSS_QUALITY_MIN_SIDE (11)
#define RFN_GAUSS_QUALITY_MAX_SIDE (128)
int rfn_linext_max_frames(void);
int rfn_linext_max_blocks(void);
int rfn_gauss_quality_min_side(void);
int rfn_gauss_quality_max_side(void);
int rfn_linext_train_f32(const float* x, long seq_stride, long frame_stride, int start, const float* w,
                         const float* bias, float* partials, long partial_floats, float* out, int B, int T, int n,
                         long CHW, rfn_stream_t stream);
int rfn_linext_rollout_f32(const float* x, long seq_stride, long frame_stride, int start, const float* w,
                           const float* bias, float* out, int B, int T, int n, int P, long CHW, rfn_stream_t stream);
int rfn_gauss_quality_f32(const float* pred, const float* truth, float* ssim, float* mse, int N, int C, int H, int W,
                          float scale, float lo, float hi, rfn_stream_t stream);

/* ---- pixel log-likelihoods of the baselines' importance-weighted bound, csrc/pixel_loglik.hip  (forward only; DESIGN.md
 * section 29 is the contract).
 *
 * rfn_pixel_loglik_f32  (VRNN/VRNN.py:400-415, SVG/SVG.py:371-380 inside :344-385, SRNN/SRNN.py:482-579 of the reference:
 *   `lpx_Gz_obs` of one time step for all K inner samples at once, in place of x.repeat(K, ...), the torch.distributions
 *   log_prob chain and batch_reduce).  pred: [R, N] dense, row r = k*B + b;  target: B rows of N floats, target_stride
 *   floats apart (>= N), row r of pred is scored against row r % B: the frame is never repeated in memory;  noise: NULL
 *   or [R, N] dense, added to the target of its row (the "gaussian" dequantisation x + u, one draw per inner sample);
 *   out: [R], out[r] = sum_n l(pred[r, n], x[r, n]) with x = target (+ noise) and, by `mode`,
 *     RFN_PIXEL_LOGLIK_BERNOULLI  l = x log(pc) + (1 - x) log1p(-pc),  pc = min(max(p, 2^-23), 1 - 2^-23)
 *                                 (torch.distributions.Bernoulli(probs=p).log_prob(x) written out; x need not be binary)
 *     RFN_PIXEL_LOGLIK_GAUSSIAN   l = -(x - p)^2 / (2 scale^2) - log(scale) - log(2 pi) / 2
 *     RFN_PIXEL_LOGLIK_MSE        l = -(p - x)^2
 *   `scale` is read by GAUSSIAN only (positive and finite).  A term's sums, differences, products and squares are fp64
 *   operations on the fp32 inputs, the two logs are the accurate fp32 logf / log1pf, and the term is rounded to fp32
 *   once.  Summation order, a function of N alone: one workgroup of 256 lanes per row; the row is cut into groups of four
 *   consecutive elements (the last may be short), lane t takes groups t, t + 256, t + 512, ... and adds their terms to
 *   an fp32 sum that starts at +0, in element order; the 64 sums of each wavefront are combined by the xor butterfly
 *   (offsets 32, 16, 8, 4, 2, 1), and the four wavefront sums w0..w3 are added as ((w0 + w1) + w2) + w3.  The longest
 *   chain has A(N) = L - 1 + 9 additions, L = the elements of lane 0 (48 at N = 12288).  A group is read as one 16-byte
 *   load per operand when the row's bases in pred, target and noise are all 16-byte aligned (decided per row), else as
 *   single floats: the same values in the same order either way.  No atomics; out[r] depends on row r, its target row
 *   and N alone, not on R, on the other rows of the call or on the launch (rows beyond the grid are taken by a
 *   grid-stride loop).  Any N >= 1, any 4-byte aligned bases, 0 <= R <= 2^31 - 1 (R = 0: nothing is launched), R a
 *   multiple of B.  One launch.  Returns -1 for a bad size, -2 for an unknown mode, -3 for a bad scale, -4 for a NULL or
 *   misaligned pointer; nothing is launched then.
 *
 * rfn_normal_logvar_pair_f32  (SVG/SVG.py:344-385: `Normal(mu, exp(logvar / 2)).log_prob(z).sum(-1)` of the prior and of
 *   the posterior of one inner sample).  Six [B, Z] dense inputs, out_a / out_b: [B];
 *   out_a[b] = sum_j -logvar_a[b,j] / 2 - (z_a[b,j] - mu_a[b,j])^2 exp(-logvar_a[b,j]) / 2 - log(2 pi) / 2, out_b likewise:
 *   the caller chooses which z goes with which distribution.  Terms in fp64 (fp64 exp), rounded to fp32 once.  One
 *   wavefront per row and distribution: lane l adds the terms j = l, l + 64, ... in index order, then the xor butterfly.
 *   No atomics, one launch for both.  Returns -1 for a bad size, -2 for a NULL pointer.
 * (The three modes are written in parentheses, like RFN_LINEXT_MAX_FRAMES: the binding mirrors plain-integer defines
 * only; rfn_hip/pixel_loglik.py keeps the names in this order.) */
#define RFN_PIXEL_LOGLIK_BERNOULLI (0)
#define RFN_PIXEL_LOGLIK_GAUSSIAN (1)
#define RFN_PIXEL_LOGLIK_MSE (2)
int rfn_pixel_loglik_f32(const float* pred, const float* target, long target_stride, const float* noise, float* out,
                         long R, int B, long N, int mode, double scale, rfn_stream_t stream);
int rfn_normal_logvar_pair_f32(const float* mu_a, const float* logvar_a, const float* z_a, const float* mu_b,
                               const float* logvar_b, const float* z_b, float* out_a, float* out_b, int B, int Z,
                               rfn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RFN_HIP_H */
