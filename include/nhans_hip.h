/* nhans_hip.h -- C ABI of libnhans_hip.so, the MI355X (gfx950) implementation of the N-HANS
 * per-frame inference hot path.
 *
 * The reference has no FFI/plugin interface: its hot path is a chain of TensorFlow graph calls
 * inside apply_snc / apply_separator.  Each entry point below replaces one link of that chain
 * (citations relative to /root/reference; SN = N_HANS___Selective_Noise, SS = N_HANS___Source_Separation):
 *
 *   nhans_stft_features  <- tf.signal.stft + log(abs+1e-5) + angle       SN/apply.py:368-375  (SS/apply.py:316-322)
 *   nhans_embed          <- model(): 'embedding' scopes                   SN/main.py:190-216   (SS/main.py:206-229)
 *   nhans_mask_net       <- strided_crop + minibatch loop + model() stack SN/apply.py:378,398-450, SN/main.py:219-242
 *                           (tensor contract: feed mixedph/noise*contextph, fetch add_72:0, SN/apply.py:434-446)
 *   nhans_istft          <- recover_samples_from_spectrum                 SN/apply.py:189-204  (SS/apply.py:158-171)
 *   nhans_enhance_clips  <- apply_snc / apply_separator after handle_signals  SN/apply.py:368-458 (SS/apply.py:316-393)
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every int-returning function gives 0
 * on success or a negative NHANS_E* code, with a message in nhans_last_error() (thread-local).
 * `*_dev` pointers are device (HBM) addresses owned by the caller; `*_host` pointers are host
 * arrays.  `stream` is a hipStream_t (0 = default stream); all work is enqueued on it and the
 * functions do not synchronise.  Caller-owned memory: a call writes the counted elements of each clip's room -- the
 * elements its section documents -- and nothing else of the caller's memory, whatever the alignment of the pointers and
 * however much larger a room is than its count, and it reads no element outside the ranges its offsets name
 * (tests/test_gpu_memory_contract.py holds every entry point to this).  The library owns only its context: folded weights and a
 * workspace that grows on demand.  One context per (device, model); a context is not
 * thread-safe, distinct contexts are independent (also on different devices of one process).
 * Consecutive calls on one context share its workspace: the library orders them itself -- a call
 * on another stream than the previous one first makes its stream wait (hipStreamWaitEvent) for the
 * previous call's work -- so results never depend on the caller's choice of streams, but two calls
 * on one context never overlap either; use one context per concurrent stream for that.
 * A kernel launch the runtime rejects (invalid grid, LDS request, ...) is reported by the entry
 * point that issued it as NHANS_EHIP, naming the kernel; nothing runs on unlaunched results.
 *
 * Ragged batches: clip c owns samples [sample_offsets[c], sample_offsets[c+1]) of the wav
 * buffer and frames [frame_offsets[c], frame_offsets[c+1]) of every [T_total, 201] tensor, with
 * T_c = nhans_num_frames(n_c) = 1 + (n_c - 400) / 160 for n_c >= 400 (the caller has already
 * applied the reference's normalise + tail-trim, SN/apply.py:150-161).  A batch may hold any number of
 * frames (64-bit offsets between clips); ONE clip is limited to 5,000,000 frames (13.9 hours: offsets inside a
 * clip are 32-bit) and a longer one is refused with NHANS_EINVAL.
 */
#ifndef NHANS_HIP_H
#define NHANS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NHANS_ABI_VERSION 5

#define NHANS_DENOISER 0   /* SN model: emb_a = positive context (--pos), emb_b = negative (--neg) */
#define NHANS_SEPARATOR 1  /* SS model: emb_a = interferer  (--neg),      emb_b = target   (--pos) */

#define NHANS_OK 0
#define NHANS_EINVAL (-1)   /* bad argument / malformed blob */
#define NHANS_EHIP (-2)     /* HIP runtime error */
#define NHANS_ENOMEM (-3)   /* workspace allocation failed */
#define NHANS_ESHORT (-4)   /* a conditioning recording yields fewer than 200 frames */

/* sticky device-side status bits, see nhans_take_status() */
#define NHANS_STATUS_SATURATED 1   /* precision 1: an activation did not fit the f16 range (|v| >= 65504 or NaN)
                                      and was clamped -- the outputs of the calls since the last
                                      nhans_take_status() are not trustworthy; rerun them with precision 0,
                                      best inside a "calibrate" bracket so that the exponents follow */

/* tensors of the network that carry an activation exponent (see "calibrate" below): tower block b conv1 / conv2
 * outputs at 2b / 2b+1 (b < 4), stack block b conv1 / conv2 outputs at 8+2b / 8+2b+1 (b < 8), last_conv at 24 */
#define NHANS_NUM_ACTIVATIONS 25

#define NHANS_WIN 400
#define NHANS_HOP 160
#define NHANS_BINS 201
#define NHANS_MIX_WIN 35
#define NHANS_CTX_FRAMES 200
#define NHANS_EMB 512

typedef struct nhans_ctx nhans_ctx;

int nhans_abi_version(void);
const char* nhans_last_error(void);

/* frames of an n-sample (already trimmed or not) signal: 0 if n < 400, else 1 + (n-400)/160 */
int64_t nhans_num_frames(int64_t nsamples);

/* Build a context from the folded-weights blob produced by nhans_amd.fold.fold_weights()
 * (format documented in n-hans_amd/fold.py).  The blob is copied to the device.  If the blob carries split-f16
 * weights, the activation exponents are calibrated here on a built-in two-second signal (one small pass of the whole
 * path in f32 mode; see "calibrate").  The blob's header carries the version of the packing conventions
 * (fold.BLOB_VERSION, 2 since ABI 4); a blob of another version is refused with NHANS_EINVAL -- it would load and compute
 * wrong results -- and the message says to fold the weights again. */
int nhans_create(int model_kind, const void* folded_blob, size_t nbytes, int device_id, nhans_ctx** out);

/* (ABI 5) The same with the activation exponents handed in -- the NHANS_NUM_ACTIVATIONS values a previous context
 * reported for THIS blob (nhans_get_activation_exponents after nhans_create): the calibration pass is skipped, which
 * with a cached folded blob (nhans_amd/blobcache.py) is what brings a cold one-file `nhans_denoiser` call -- the
 * reference's normal use, SN/apply.py:478-527: one process per file -- under a second.  act_exp == NULL: as nhans_create.
 * Exponents outside [-60, 60] or n_exp != NHANS_NUM_ACTIVATIONS: NHANS_EINVAL.  Wrong exponents cannot corrupt results
 * silently: too small raises NHANS_STATUS_SATURATED (Engine redoes the batch in f32), too large costs accuracy bits. */
int nhans_create_ex(int model_kind, const void* folded_blob, size_t nbytes, int device_id, const int* act_exp, int n_exp,
                    nhans_ctx** out);
void nhans_destroy(nhans_ctx* ctx);

/* Options: "lookahead" (L, 0..17 frames, default 17: what every release so far computed, bit for bit.  Frame g of a clip
 *           of T frames is computed with its clip length taken as T_g = min(T, g + L + 1): the rows of its 35-row window
 *           at clip positions >= T_g read as 0.0, the network's own end-of-clip behaviour -- strided_crop, SN/apply.py:
 *           170-186 -- applied L frames behind the frame; centre row, phase, iSTFT and pairing are unchanged.  Applies to
 *           nhans_mask_net, nhans_enhance_clips and the three debug taps of the stack; the only device-side difference is
 *           the per-frame length table.  This is the offline twin of a live stream's look-ahead, "Look-ahead" below:
 *           online and live objects carry their own L and ignore this option.  Outside 0..17: NHANS_EINVAL),
 *          "frames_per_chunk" (mask-net frame windows per pass, 1..4769 -- the conv kernels address a pass's
 *           largest tensor, frames x 35 x 201 x 64 elements, with 32-bit offsets; default 3776: 24 GB of workspace
 *           for batches that large, 6.4 MB per frame, chosen so that the launches fill whole waves of 256 workgroups),
 *          "contexts_per_chunk" (embedding-tower images per pass, default 64),
 *          "profile" (1: time every kernel launch with hipEvents on the launch stream),
 *          "precision" (0: exact f32 matrix-core path, default; 1: split-f16 x3 -- every operand is
 *           carried as hi+lo f16 and multiplied with three f16 MFMAs into an f32 accumulator;
 *           FP32-class accuracy, activations must stay below the f16 range 65504),
 *          "conv_variant" (-1: automatic, default; 0: register-staged 128-pixel kernel; 1: LDS-DMA
 *           256-pixel kernel; 2: halo-reuse kernel with producer/consumer waves where the conv
 *           allows it (512-pixel tiles for the 64-channel convs), the same pipeline with one staged image per tap
 *           for the strided / VALID convs with >= 128 output channels, else 1 -- same results
 *           within rounding, different speed).
 *          "epilogue_wide" (1, default: split-f16 epilogues move 8 channels = 16-byte pieces per thread;
 *           0: 4 channels -- identical bits, kept for A/B),
 *          "consumer_interleave" (1, default: the MFMA waves of the halo kernel issue their LDS operand
 *           reads between their MFMAs, one behind each of the first MFMAs of a half-tap; 2: spread evenly over the
 *           half-tap; 0: read block then MFMA block -- identical bits, kept for A/B),
 *          "calibrate" (activation exponents of the split-f16 mode: every stored tensor is kept as x * 2^-e with one
 *           integer e per tensor, so that models whose activations are far from O(1) -- no BatchNorm statistics can
 *           promise that -- stay inside the f16 range instead of tripping NHANS_STATUS_SATURATED; scaling by a power
 *           of two is exact, the arithmetic is otherwise bit for bit that of e = 0.  1: start recording the largest
 *           |x| of every tensor in the calls that follow (any precision; precision 0 cannot saturate and is what a
 *           calibration on own data should use); 0: stop and set every e so that the recorded maximum is stored as
 *           at most 2^8; 2: stop and only RAISE exponents (what a caller does after a saturated batch: rerun it at
 *           precision 0 inside the bracket -- that is the correct result for it -- and go on at precision 1);
 *           3: stop and discard (the recorded pass failed).  Stopping synchronises the device.  A tensor the pass never
 *           wrote keeps its exponent.  A maximum that is not finite is refused with NHANS_EINVAL by 0 and ignored by 2
 *           (a NaN / Inf INPUT raises the flag as well and says nothing about the range).  Exponents raised after a
 *           saturated batch persist: the bits of later batches depend on that history -- set them explicitly
 *           (nhans_set_activation_exponents) where ranks or runs must agree bit for bit.),
 *          "winograd" (1, default: in split-f16 mode the stride-1 4x4 convs of the residual stack run as 1-D
 *           Winograd convolutions F(5,4) along the image width, 2.5 x fewer matrix-core MACs -- conv_wino.hip;
 *           0: the direct kernels for every conv -- results agree to ~1e-5 on the logits),
 *          "winograd_f32_tensors" (1, default: with the Winograd form, the stack tensors that only Winograd launches read
 *           are stored f32 NHWC instead of split NHWC -- same size, same scaled values, less work in the transform;
 *           0: every tensor split -- results agree to ~1e-6 on the logits; 2: a TEST value -- f32 storage whatever the
 *           readers are: a reader that is not a Winograd launch then refuses, the call returns NHANS_EHIP and nothing is
 *           computed on a wrong layout; 3: a TEST value -- only the output of resblock1_2 is f32: its conv2 then has a
 *           split residual and an f32 output, the one layout pair the Winograd epilogue does not implement, and the launch
 *           is refused the same way.  After a refused or failed launch nothing further of that pass is launched.),
 *          "stream_1x1" (1, default: the stand-alone 1x1 strided `_transform` conv of resblock2_1 -- an HBM stream, 1.75 GB in and
 *           3.5 GB out per pass -- runs on its own streaming kernel, conv_1x1_stream.hip; 0: on the generic implicit-GEMM kernel.
 *           Identical bits),
 *          "row_split" (1, default: in split-f16 mode the 3x3 convs of resblock3 and resblock4 -- 9 x 51 and 5 x 26 images, where
 *           the top filter row of the first output row and the bottom filter row of the last read nothing but SAME padding --
 *           run as one launch per class of output rows (top, interior, bottom), each with only the filter rows that touch the
 *           image: 7 % and 13 % fewer matrix-core MACs in those convs.  0: one launch per conv.  2: a measurement value --
 *           every conv of the stack that can be split is, the strided ones with 4 % to gain included.  Identical bits:
 *           the filter rows left out added exact zeros; the profile's `flops` of the class launches sum to the single
 *           launch's, `mfma_flops` is what ran),
 *          "split_k" (1, default: the launches too small to fill the chip -- the head's dense layer, the embedding tower
 *           at a few clips -- run one workgroup per (tile, K group) through a scratch buffer; 0: every workgroup walks
 *           its K groups itself.  The groups and the order of the additions depend on the layer only: identical bits),
 *          "bss_group_bytes" (2147483648, default: the bytes of workspace the Gram factors of one group of nhans_bss_eval's
 *           clips may take together; a group holds at least one clip.  A debug value: the grouping changes no bit of any
 *           record, a small value only forces more groups),
 *          "phase_iters" (0, default, ... 256: Griffin-Lim iterations of nhans_enhance_clips on the denoised rows before
 *           their iSTFT -- "Phase refinement" below; online and live objects ignore it),
 * (A `make DEV=1` build adds "debug_cycles_ptr" and the NHANS_ABLATE environment switch used by tools/; the default build has no developer hooks and reads no environment.)
 * Besides the workspace a context holds split-K scratch for the few launches that are too small to fill the chip (the
 * head's dense layer, the embedding tower at a few clips): allocated on the first such launch, sized by what the launches
 * need (32 MB ... 384 MB; 120 MB for the head at the default 3,776 frame windows per pass).  If that allocation fails
 * the launches run unsplit -- same bits, slower -- and nothing is reported. */
int nhans_set_option(nhans_ctx* ctx, const char* key, int64_t value);

/* Activation exponents (see "calibrate"): n must be NHANS_NUM_ACTIVATIONS.  Tensors that share one accumulator -- the
 * input of a channel-changing block and its conv1 output -- are kept on one exponent (the larger); `get` returns what
 * is in effect.  nhans_get_activation_amax: the maxima the last finished calibration recorded. */
int nhans_set_activation_exponents(nhans_ctx* ctx, const int* e, int n);
int nhans_get_activation_exponents(nhans_ctx* ctx, int* e_out, int n);
int nhans_get_activation_amax(nhans_ctx* ctx, float* amax_out, int n);

/* Bytes of device workspace the context would hold for a batch of this shape. */
size_t nhans_workspace_bytes(nhans_ctx* ctx, int64_t total_frames, int nclips);

/* wav -> log-magnitude and phase.  max_frames_per_clip > 0 truncates every clip to its first
 * frames (used for the 200-frame conditioning contexts, SN/apply.py:381).  Outputs are
 * [sum_c min(T_c, max), 201] float32; phase_dev may be NULL.  With max_frames_per_clip > 0 a clip that has fewer frames
 * is refused with NHANS_ESHORT and nothing is written.  A clip may carry up to 159 samples behind its last frame
 * (they are not read into any frame).  Any finite float32 samples: every log-magnitude is finite and every phase lies in
 * [-pi, pi]; atan2(0, 0) = 0.  A bin whose real and imaginary parts are both below the smallest normal float32 (1.18e-38)
 * has zero magnitude to the hardware reciprocal: its phase is that of the axis of its larger part (0, +-pi/2 or +-pi), not
 * the angle between the two -- under the 1e-5 floor such a bin's log-magnitude is ln 1e-5 either way. */
int nhans_stft_features(nhans_ctx* ctx, const float* wav_dev, const int64_t* sample_offsets_host,
                        int nclips, int max_frames_per_clip, float* logmag_dev, float* phase_dev,
                        void* stream);

/* Embedding tower: n context images [n,200,201] -> [n,512]. */
int nhans_embed(nhans_ctx* ctx, const float* ctx_logmag_dev, int n, float* emb_out_dev, void* stream);

/* Conditioned residual stack + head over every frame of every clip.  logmag [T_total,201];
 * emb_a/emb_b [nclips,512] in resnet_block argument order (see NHANS_DENOISER/SEPARATOR).
 * logits_out_dev (nullable) receives `out` = last_dense output; denoised_out_dev receives
 * logmag + out (the reference's add_72:0).  Sliding 35-frame windows are gathered on the fly
 * with rows outside the clip equal to 0.0 (SN/apply.py:170-186). */
int nhans_mask_net(nhans_ctx* ctx, const float* logmag_dev, const int64_t* frame_offsets_host,
                   int nclips, const float* emb_a_dev, const float* emb_b_dev,
                   float* logits_out_dev, float* denoised_out_dev, void* stream);

/* exp/polar -> 400-point inverse real FFT -> synthesis window -> overlap-add.  Clip c writes
 * (T_c-1)*160+400 samples at wav_out_dev + out_offsets_host[c] (out_offsets_host has nclips + 1 entries).  The phases
 * at bins 0 and 200 are used through their cosine only, as a real inverse FFT does.  Phases are expected in [-pi, pi],
 * both ends included: there the output is within float32 rounding of the float64 result.  Larger angles are accepted and
 * not reduced first; the angle goes to the hardware sine in revolutions rounded to float32, so each phase is off by up to
 * half an ulp of |phase / 2 pi| -- 2^-23 revolutions = 7.5e-7 rad between 4 pi and 8 pi.  Log-magnitudes from ln 1e-5 - 20 to 16 are covered by the
 * tests; exp(logmag) must stay a finite float32. */
int nhans_istft(nhans_ctx* ctx, const float* logmag_dev, const float* phase_dev,
                const int64_t* frame_offsets_host, int nclips, const int64_t* out_offsets_host,
                float* wav_out_dev, void* stream);

/* Whole hot path for a ragged batch.  Mixture clips must be trimmed so (n-400)%160 == 0;
 * context clips need >= 32,240 samples (only their first 200 frames are used).  ctx_a/ctx_b
 * follow the emb_a/emb_b convention.  denoised_wav_dev and mixed_wav_dev (nullable: the
 * reference's *mixed_processed.wav round trip) use the mixture's sample offsets.  Optional
 * taps (nullable): logmag_out_dev/phase_out_dev/logits_out_dev [T_total,201], emb_out_dev
 * [2*nclips,512] (a-rows then b-rows). */
int nhans_enhance_clips(nhans_ctx* ctx, const float* mix_wav_dev, const int64_t* mix_offsets_host,
                        int nclips, const float* ctx_a_wav_dev, const int64_t* ctx_a_offsets_host,
                        const float* ctx_b_wav_dev, const int64_t* ctx_b_offsets_host,
                        float* denoised_wav_dev, float* mixed_wav_dev, float* logmag_out_dev,
                        float* phase_out_dev, float* logits_out_dev, float* emb_out_dev, void* stream);

/* Debug tap: run the stack on `nframes` frame windows starting at global frame `frame0` and copy
 * the NHWC output of main block `block` (0..7; 8 = last_conv) to out_dev. */
int nhans_debug_block_output(nhans_ctx* ctx, const float* logmag_dev, const int64_t* frame_offsets_host,
                             int nclips, const float* emb_a_dev, const float* emb_b_dev,
                             int64_t frame0, int nframes, int block, float* out_dev, void* stream);

/* Debug taps on every stored tensor, in the numbering of NHANS_NUM_ACTIVATIONS, as plain f32 NHWC.  Both run the
 * production launch sequence (same plan for the whole stack, same layouts, chunking, variant, Winograd and split-K
 * choices as nhans_mask_net / nhans_embed with the options in effect) and only convert the finished buffer.
 * nhans_debug_activation: stack tensors, index 8 .. 24 (block b conv1 output -- after conditioning, BatchNorm and ReLU --
 * at 8+2b, block output at 8+2b+1, last_conv at 24), for frames [frame0, frame0 + nframes) of the ragged batch, in passes of
 * "frames_per_chunk" frame windows counted from frame0; out_dev [nframes, Ho, Wo, C].
 * nhans_debug_tower_activation: tower tensors, index 0 .. 7 (block b conv1 output at 2b, block output at 2b+1), for n
 * context images [n,200,201] in passes of "contexts_per_chunk"; out_dev [n, Ho, Wo, C].
 * An index outside the range, nframes < 1, n < 1, a frame range outside the batch or a null pointer: NHANS_EINVAL. */
int nhans_debug_activation(nhans_ctx* ctx, const float* logmag_dev, const int64_t* frame_offsets_host,
                           int nclips, const float* emb_a_dev, const float* emb_b_dev,
                           int64_t frame0, int nframes, int index, float* out_dev, void* stream);
int nhans_debug_tower_activation(nhans_ctx* ctx, const float* ctx_logmag_dev, int n, int index, float* out_dev,
                                 void* stream);

/* Waits for `stream`, then returns the context's sticky status bits (NHANS_STATUS_*) in
 * *flags_out and clears them.  The hot-path calls are asynchronous, so conditions detected on the
 * device (split-f16 activation overflow) cannot be part of their return code; a caller that uses
 * precision 1 on weights it has not validated calls this once per batch. */
int nhans_take_status(nhans_ctx* ctx, int* flags_out, void* stream);

/* Self-test of the launch-error path (needs no context): launches a trivial kernel on the current
 * device with `dynamic_lds_bytes` of dynamic LDS.  Returns NHANS_OK if the launch was accepted,
 * NHANS_EHIP (with the runtime's message in nhans_last_error()) if not -- e.g. for a request above
 * the 160 KB a gfx950 CU has, or when no HIP device is present. */
int nhans_debug_launch_probe(size_t dynamic_lds_bytes, void* stream);

/* Measures what the f16 matrix pipes of the current device sustain at its socket power cap (needs no
 * context): back-to-back independent v_mfma_f32_32x32x16_f16 -- the instruction the split-f16 conv kernels
 * issue -- on pseudo-random register operands, no LDS, no memory, launch after launch for `seconds`
 * (0 < seconds <= 60; blocks the calling thread).  *sustained_tflops = mean rate over the second half of the
 * launches, *first_tflops (nullable) = the first launch (boost clock), *launches (nullable) = launches run.
 * bench.py reports it as roofline.peak_at_power_cap: the data-sheet 2.5 PFLOP/s is reached only on operands
 * that do not toggle the multipliers.  Replaces nothing in the reference: measurement. */
int nhans_debug_mfma_ceiling(double seconds, void* stream, double* sustained_tflops, double* first_tflops,
                             int* launches);

/* Host helper (no device involved): the row classes "row_split" launches a conv segment by.  Input height H, filter height
 * KH, row stride and top padding pt (output height ceil(H / stride)): output row ho reads input rows ho*stride - pt + kh, and
 * consecutive output rows with the same range of kh inside [0, H) form a class.  Writes (oh0, rows, kh0, KH') per class to
 * out[4 * cap] in row order and returns their number -- a class launch has Ho = rows, KH = KH' and pt' = pt - kh0 -
 * oh0*stride.  0: some output row reads padding only, such a conv is not split.  Bad arguments or more classes than
 * `cap`: NHANS_EINVAL. */
int nhans_debug_row_classes(int H, int KH, int stride, int pt, int* out, int cap);

/* Host helper (no device involved): the batch nhans_create calibrates the activation exponents on (see "calibrate") -- two
 * mixtures of lengths_out[0] samples each, written one after the other to mix_out, and their two pairs of context
 * recordings of lengths_out[1] samples each, clip 0's then clip 1's, in ctx_a_out and ctx_b_out.  The built-in
 * calibration is a "calibrate" bracket at precision 0 round nhans_enhance_clips of exactly these arrays (the same
 * function fills them), so a caller can repeat it and compare.  The three arrays all null: only the lengths are
 * written.  lengths_out null, or some arrays null and some not: NHANS_EINVAL. */
int nhans_debug_builtin_batch(float* mix_out, float* ctx_a_out, float* ctx_b_out, int64_t* lengths_out);

/* Host helper (no device involved): CRC-32C (Castagnoli) of a host buffer continued from `crc`
 * (0 to start).  TensorFlow checkpoint bundles store crc32c::Mask() of it per tensor; tfbundle.py
 * verifies the 116 MB data shard with it (BundleEntryProto field 6 of the reference's shipped trained_model .index files). */
uint32_t nhans_crc32c(uint32_t crc, const void* data_host, size_t nbytes);

/* ---- Online enhancement: live recordings pushed piece by piece, bit-identical to offline ----------------------------
 * One object holds S live recordings ("online streams", not to be confused with the hipStream_t `stream` argument) of
 * one context; every push moves all S through the GPU together.  Every output frame depends only on its 35-frame window
 * of the log-magnitude spectrogram (17 frames back, 17 ahead) and on the two conditioning embeddings, the STFT computes
 * each frame on its own and the iSTFT sums each output sample from its <= 3 frames in a fixed order, so the online
 * output is BIT FOR BIT what nhans_enhance_clips computes for the same samples trimmed by the offline rule.
 *
 * Output contract, per online stream.  N = samples pushed so far, T = nhans_num_frames(N), L = the slot's look-ahead (17
 * unless nhans_online_set_lookahead said otherwise), R = max(0, T - L) (the frames whose L look-ahead rows exist; T once
 * the stream has ended), P = R rounded down to an even number.  Until the stream ends, the samples emitted
 * so far number 160 * P; once it has ended they number (T - 1) * 160 + 400, or 0 if T = 0 -- the offline output length
 * of the input trimmed to whole frames (the samples of an incomplete last hop are dropped, as offline).  P is even
 * because the offline iSTFT transforms frames in pairs (2k, 2k+1) of the clip: a frame is synthesised with the offline
 * bits once its partner exists or the stream has ended.  Algorithmic latency: the L-frame look-ahead plus one window,
 * (160 L + 400) / 16 kHz = 10 L + 25 ms, +- 10 ms for where a sample falls in its hop and for the pair rule: 185 - 205 ms
 * at the default L = 17, 35 - 55 ms at L = 2, 15 - 35 ms at L = 0.
 *
 * Look-ahead.  With L < 17 frame g is computed as soon as frame g + L exists, with its clip length taken as g + L + 1 (or
 * the stream's final length, if that is smaller): the output is BIT FOR BIT nhans_enhance_clips under option "lookahead"
 * = L ("den_L").  den_L is a function of the recording and L alone, never of the cutting: a frame computed in a push that
 * already holds more than L rows behind it still reads them as 0.0.  What a small L costs in quality is a property of the
 * trained model; nothing in this library measures it.  The carried state needs no more room: T - lo <= L + 24 <= 41 rows
 * of spectrogram and R - S0 <= 24 denoised rows for every L <= 17.
 *
 * Calls on the context stay ordered as every other call is (see the top of this file): offline calls and other online
 * objects of the same context may be interleaved with pushes.  A push whose ready frames exceed "frames_per_chunk" runs
 * the stack in several passes inside the call.  The object owns its state (about 89 KB per online stream, twice: the
 * slot a push reads and the slot it writes) and the embeddings; the context's workspace serves each push while it runs.
 * Objects are closed (nhans_online_close) BEFORE nhans_destroy(ctx).
 *
 * Slots.  A slot is one of the S stream positions of an object, and it outlives the streams that pass through it:
 *   open       nhans_online_open: S conditioned slots, each an open stream of 0 samples.  nhans_online_open_slots: S
 *              unconditioned slots, no tower run (what a long-lived service object starts as).
 *   join       nhans_online_restart (the slot becomes an open stream of 0 samples) + nhans_online_set_context or
 *              nhans_online_set_embeddings (the slot's conditioning; the slot is "conditioned" from then on).
 *   run        pushes.  A slot nobody uses gets 0 samples in every push and reports 0: it adds no frames, hence no STFT,
 *              stack or iSTFT work; only the per-pass conditioning kernel still touches all S embedding row pairs.
 *   leave      end_host in a push (the tail is flushed, the output has the offline length), or nhans_online_restart
 *              (the samples not emitted yet are dropped: the output is the first 160 * P samples of the offline one).
 *   again      a slot that has ended, or was abandoned, is taken over by the next join; conditioning survives a restart.
 * Pushing samples or an end to an unconditioned slot is NHANS_EINVAL.  nhans_online_out_counts follows the slot's
 * current stream.  The slot count is fixed when the object is opened.  A slot's look-ahead survives a restart, as its
 * conditioning does.
 *
 * Changing the conditioning of a running stream (the set functions alone, no restart).  Let R be the number of frames of
 * the slot's stream already computed when the call is made (R above; T once the stream has ended): the call reports it.
 * Frames >= R are computed with the new conditioning, frames < R have used the old one.  The iSTFT packs frames
 * (2k, 2k+1) of a stream into one complex transform, so a frame's waveform bits can depend on its partner's data
 * (about 1e-7).  With B = R rounded down to even, B' = R rounded up to even, and den1 / den2 the outputs of
 * nhans_enhance_clips for the whole trimmed recording under the old / the new conditioning:
 *   - output samples [0, 160 * B) are bit for bit den1;
 *   - output samples [160 * B' + 240, end) are bit for bit den2;
 *   - R = 0: the whole output is den2.  R = the stream's final frame count: the whole output is den1;
 *   - the at most 560 samples between are finite and otherwise unspecified (a cross-fade of the two by the synthesis
 *     window, up to the pair effect);
 *   - the mixed round trip does not depend on conditioning and stays bit for bit the offline one. */
typedef struct nhans_online nhans_online;

/* Opens an object of `nstreams` (>= 1) online streams.  Stream i is conditioned on clips i of ctx_a / ctx_b, with the
 * rules of nhans_enhance_clips: at least 32,240 samples (else NHANS_ESHORT), only the first 200 frames used, the same
 * (a, b) order.  The embedding towers run here, once per stream.  want_mixed != 0: pushes also write the
 * *mixed_processed round trip. */
int nhans_online_open(nhans_ctx* ctx, int nstreams, const float* ctx_a_wav_dev, const int64_t* ctx_a_offsets_host,
                      const float* ctx_b_wav_dev, const int64_t* ctx_b_offsets_host, int want_mixed, void* stream,
                      nhans_online** out);

/* Opens an object of `nslots` (>= 1) slots without conditioning: every slot is an open stream of 0 samples that accepts
 * only 0-sample pushes until one of the set functions below has given it conditioning.  No tower runs; the embedding
 * rows are zero-filled. */
int nhans_online_open_slots(nhans_ctx* ctx, int nslots, int want_mixed, void* stream, nhans_online** out);

/* Host only.  Slot `slot` becomes an open stream of 0 samples, whatever it was: ended, or still running (its samples
 * not emitted yet are dropped).  Its conditioning is kept.  Nothing is cleared on the device: a fresh stream reads none
 * of the old state. */
int nhans_online_restart(nhans_online* obj, int slot);

/* Conditions slot `slot` on two recordings (rules of nhans_online_open: at least 32,240 samples each, else
 * NHANS_ESHORT; the first 200 frames; the same (a, b) order): STFT and embedding tower for this slot alone.
 * *first_frame_out (nullable) receives R of the section above: frames >= R of the slot's stream use the new
 * conditioning.  On any error the slot's conditioning and stream are unchanged. */
int nhans_online_set_context(nhans_online* obj, int slot, const float* ctx_a_wav_dev, int64_t na,
                             const float* ctx_b_wav_dev, int64_t nb, void* stream, int64_t* first_frame_out);

/* The same with two ready [512] rows (what nhans_embed returns), so that the towers can run elsewhere -- another
 * context, another hipStream_t -- and a join does not stall this context's pushes. */
int nhans_online_set_embeddings(nhans_online* obj, int slot, const float* emb_a_dev, const float* emb_b_dev,
                                void* stream, int64_t* first_frame_out);

/* nhans_online_restart and the two set functions make the last push final: nhans_online_rewind after one of them
 * returns NHANS_EINVAL until the next push.  A slot out of range, a NULL object or a NULL pointer that is needed:
 * NHANS_EINVAL with the function's name in nhans_last_error(). */

/* Appends in_offsets_host[i+1] - in_offsets_host[i] (>= 0) normalised float32 samples of in_dev to stream i; end_host
 * (nullable) != 0 ends stream i after them.  Writes every output sample that is now final: out_counts_host[i] samples
 * at den_out_dev + out_offsets_host[i] (and, with want_mixed, at mixed_out_dev + out_offsets_host[i]); the caller's
 * room out_offsets_host[i+1] - out_offsets_host[i] must hold them (nhans_online_out_counts), else NHANS_EINVAL.
 * Pushing to an ended stream, samples or an end to an unconditioned slot, a negative count or a NULL that is needed:
 * NHANS_EINVAL, and nothing changes. */
int nhans_online_push(nhans_online* obj, const float* in_dev, const int64_t* in_offsets_host, const int* end_host,
                      float* den_out_dev, float* mixed_out_dev, const int64_t* out_offsets_host,
                      int64_t* out_counts_host, void* stream);

/* The counts a push of in_counts_host[i] samples (end_host nullable) would report, on the host, without touching the
 * device: what a caller sizes its output buffers with. */
int nhans_online_out_counts(const nhans_online* obj, const int64_t* in_counts_host, const int* end_host,
                            int64_t* out_counts_host);

/* Undoes the most recent push -- device state, sample / frame counts and ended flags -- so that it can be redone (a push
 * that raised NHANS_STATUS_SATURATED at precision 1 is redone at precision 0 inside a "calibrate" bracket).  Once per
 * push: a second rewind, one before any push, or one after a restart / set call that followed the push, returns
 * NHANS_EINVAL.  A rewind never brings back a stream that nhans_online_restart replaced. */
int nhans_online_rewind(nhans_online* obj);

/* Host only.  The look-ahead L (0..17 frames) of slot `slot`, for its current stream and those that follow it in the slot.
 * Allowed while the slot's stream is open with 0 samples pushed (after open, or after nhans_online_restart); on a stream
 * with samples, an ended one, or L outside 0..17: NHANS_EINVAL and nothing changes.  Makes the last push final, as a
 * restart does (nhans_online_rewind).  nhans_online_out_counts and the *first_frame_out of the set calls follow it. */
int nhans_online_set_lookahead(nhans_online* obj, int slot, int lookahead);

void nhans_online_close(nhans_online* obj);

/* ---- Sample-rate conversion and the file front end -------------------------------------------------------------------
 * Everything above takes 16 kHz, already normalised float32.  Capture devices deliver int16 PCM at 48 or 44.1 kHz; the
 * reference's packaged tool converts other formats with sox before it starts (its README.md:42).  The functions below
 * are that converter on the device: stateless for files (nhans_resample), with carried state for live streams
 * (nhans_resampler_*), and the reference's peak normalisation (nhans_peak_normalise <- normalise(), SN/apply.py:150-155).
 * They were added without moving NHANS_ABI_VERSION; a caller that may meet an older library looks them up by symbol.
 *
 * For rate_in -> rate_out: g = gcd, L = rate_out / g, M = rate_in / g, half = 10 * max(L, M).  The filter is the one
 * scipy.signal.resample_poly(x, L, M) designs by default: h = firwin(2 * half + 1, 1 / max(L, M), window = ('kaiser',
 * 5.0)) * L, computed inside the library in double.  Output m of an n-sample clip is
 *     y[m] = sum_k h[m * M + half - k * L] * x[k]       0 <= m < ceil(n * L / M),   x outside [0, n) reads as 0
 * with the taps rounded to float32 once and every output ONE chain of fmaf in float32 in a fixed tap order -- the same
 * instructions whether the samples arrive in one call or piece by piece.
 * Supported pairs: one side 16000 Hz, the other 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200 or 96000 Hz;
 * 16000 -> 16000 is accepted and copies.  Any other pair: NHANS_EINVAL with the two rates in nhans_last_error(). */
#define NHANS_PCM_INT16 0
#define NHANS_PCM_FLOAT32 1
#define NHANS_RESAMPLE_QUANTISE 1     /* outputs rounded to the int16 grid (ties to even, as np.round) and clipped to
                                         [-32768, 32767], still stored as float32: what a converter that writes a 16-bit
                                         file, then reads it, hands on */
#define NHANS_NORMALISE_WRAP_INT16 1  /* the peak search takes |-32768| as -32768: np.abs of an int16 array, which is what
                                         the reference's normalise() sees for a mono 16-bit file */

/* Host only.  ceil(n * L / M), the output length of an n-sample clip; negative (NHANS_EINVAL) for an unsupported pair. */
int64_t nhans_resample_out_count(int64_t nsamples, int rate_in, int rate_out);
/* Host only.  Samples a live stream has emitted in total after nsamples inputs (the output contract below). */
int64_t nhans_resample_emitted(int64_t nsamples, int ended, int rate_in, int rate_out);
/* Host only.  The 2 * half + 1 float64 taps h (1 tap for 16000 -> 16000); returns their number, also with out == NULL. */
int nhans_resample_taps(int rate_in, int rate_out, double* out_host, int cap);

/* Ragged batch, stateless.  Clip c owns elements [in_offsets_host[c], in_offsets_host[c+1]) of in_dev (int16 or float32
 * elements by in_format) and writes its ceil(n_c * L / M) outputs at out_dev + out_offsets_host[c]; the room
 * out_offsets_host[c+1] - out_offsets_host[c] must hold them, else NHANS_EINVAL.  Clips of 0 samples are allowed. */
int nhans_resample(nhans_ctx* ctx, const void* in_dev, int in_format, const int64_t* in_offsets_host, int nclips,
                   int rate_in, int rate_out, int flags, float* out_dev, const int64_t* out_offsets_host, void* stream);

/* out = float32(double(x) / (double(peak_c) + 1e-6)) per clip, peak_c = max |x| over the clip (0 for an empty one): IEEE
 * double division, bit for bit the reference's normalise() on the same values.  out_dev == in_dev is allowed. */
int nhans_peak_normalise(nhans_ctx* ctx, const float* in_dev, const int64_t* offsets_host, int nclips, int flags,
                         float* out_dev, void* stream);

/* Down-mix of a multi-channel file: in_dev holds nchannels planes of nsamples (channel c at in_dev + c * nsamples);
 * out[i] = float32 of the mean of the planes at i, summed in double (the host converter's x.mean(axis = 1)).
 * out_dev == in_dev is allowed. */
int nhans_channel_mean(nhans_ctx* ctx, const float* in_dev, int nchannels, int64_t nsamples, float* out_dev, void* stream);

/* Live streams.  One object converts `nstreams` streams rate_in -> rate_out; per stream it keeps the last J =
 * ceil((2 * half + 1) / L) input samples and two counters.
 * Output contract: an output is emitted once every input it reads exists.  After N inputs a stream has emitted
 *     E(N) = min(ceil(N * L / M), max(0, floor((N * L - 1 - half) / M) + 1))
 * samples, and ceil(N * L / M) once it has ended (the missing inputs read as 0, as at the end of a clip).  The
 * concatenated pushes are BIT FOR BIT nhans_resample of the whole input, however it was cut, 0- and 1-sample pushes
 * included.  Added latency: half / (L * rate_in) seconds = 10 periods of the lower rate, 0.625 ms beside 16 kHz.
 * nhans_resampler_set_peak: every output becomes float32(double(y) / (peak + 1e-6)) -- the fixed-peak normalisation of a
 * live stream (there is no whole-recording peak to divide by), applied to the (quantised, with the flag) output.  It
 * holds for the outputs of the pushes that follow the call; outputs already emitted are not touched.
 * Errors follow the online functions: a stream out of range, a push after the end, a negative count, too little room
 * or a NULL that is needed: NHANS_EINVAL, and nothing changes.  Close the object BEFORE nhans_destroy(ctx). */
typedef struct nhans_resampler nhans_resampler;
int nhans_resampler_open(nhans_ctx* ctx, int nstreams, int rate_in, int rate_out, int in_format, int flags,
                         nhans_resampler** out);
int nhans_resampler_set_peak(nhans_resampler* obj, double peak);
/* Appends in_offsets_host[i+1] - in_offsets_host[i] elements to stream i (end_host nullable; != 0 ends the stream after
 * them) and writes the out_counts_host[i] samples that became final at out_dev + out_offsets_host[i]. */
int nhans_resampler_push(nhans_resampler* obj, const void* in_dev, const int64_t* in_offsets_host, const int* end_host,
                         float* out_dev, const int64_t* out_offsets_host, int64_t* out_counts_host, void* stream);
/* Host only: the counts such a push would report. */
int nhans_resampler_out_counts(const nhans_resampler* obj, const int64_t* in_counts_host, const int* end_host,
                               int64_t* out_counts_host);
/* Host only: stream i becomes an open stream of 0 samples, whatever it was. */
int nhans_resampler_restart(nhans_resampler* obj, int i);
void nhans_resampler_close(nhans_resampler* obj);

/* ---- Live PCM sessions: device-rate audio in and out, one call per push ----------------------------------------------
 * One object owns an incoming converter (rate_in -> 16000, in_format int16 or float32 elements, every converted sample
 * divided by peak + 1e-6 as nhans_resampler_set_peak does), an online object of `nslots` slots (the section "Online
 * enhancement" above: slots, joining, leaving, conditioning) and an outgoing stage (16000 -> rate_out), with the 16 kHz
 * pieces between them in device buffers of its own -- grown on demand, at least doubling, so not inside the steady state of
 * equal-sized pushes.  One push is ONE call on the context: the three stages are enqueued on the call's stream, nothing
 * is synchronised and no sample passes through the host; every count is computed on the host.  Added without moving
 * NHANS_ABI_VERSION; a caller that may meet an older library looks the functions up by symbol.
 *
 * Rates: rate_in and rate_out are each one of the rates nhans_resample converts from / to 16000 Hz, 16000 included (the
 * one-tap copy: the object always has both stages).  Anything else: NHANS_EINVAL with both rates in nhans_last_error().
 * out_format is NHANS_PCM_INT16 or NHANS_PCM_FLOAT32; out_scale is a finite double > 0.
 *
 * Output arithmetic.  den[k], mix[k]: the 16 kHz samples the online push made final (mix: the *mixed_processed round
 * trip); w: the wet factor in effect for the push that made sample k final (0 until nhans_live_set_wet).
 *   1. c[k] = den[k] + (mix[k] - den[k]) * float(w): three separately rounded float32 operations, never contracted --
 *      numpy's float32 `denoised + removed * factor` of the reference's write_snc_outputs (SN/apply.py, --compensate).
 *      With w == 0, c[k] = den[k] and mix is never read.
 *   2. y[m] = the library's one fmaf chain over c: the taps, tap order and arithmetic of nhans_resample (16000 -> rate_out).
 *   3. v = float32(double(y[m]) * out_scale).
 *   4. int16 output: rintf (ties to even), clamped to [-32768, 32767], stored as int16; float32 output: v stored.
 * The outgoing stage carries the last J values of c per slot, as a nhans_resampler carries its input: a change of w
 * applies to the 16 kHz samples later pushes make final, and the output is the conversion of the piecewise c, bit for bit.
 *
 * Output contract.  After N input samples a slot's stream has emitted nhans_live_emitted (N, ended, rate_in, rate_out) =
 *     E_out(online_emitted(E_in(N, ended), ended), ended)        (slots of look-ahead L < 17: nhans_lookahead_live_emitted)
 * samples: E_in / E_out are nhans_resample_emitted for rate_in -> 16000 and 16000 -> rate_out, online_emitted is the
 * online contract above (160 * P, or the offline length once ended).  The concatenated outputs of a stream are BIT FOR
 * BIT this offline chain, however the input was cut, 0- and 1-sample pushes included: nhans_resample (rate_in -> 16000)
 * of the whole recording; division by the fixed peak; trim to whole frames; nhans_enhance_clips with the mixed round
 * trip; steps 1 - 4 above on the whole clip.
 *
 * Errors follow the online functions: a slot out of range, a push to an ended or unconditioned slot, a negative count,
 * too little room, a NULL that is needed, a non-zero wet factor without NHANS_LIVE_WET: NHANS_EINVAL with the function's
 * name in nhans_last_error(), and nothing changes.  After a kernel launch the runtime rejects (NHANS_EHIP) the stages
 * behind it are not launched and no stage's host state has moved: the push can be repeated.
 * Close the object BEFORE nhans_destroy(ctx). */
#define NHANS_LIVE_WET 1   /* the online object also runs the mixed round trip, so that a wet/dry mix can be set */
typedef struct nhans_live nhans_live;

/* Host only.  The contract above; negative (NHANS_EINVAL) for unsupported rates or nsamples < 0. */
int64_t nhans_live_emitted(int64_t nsamples, int ended, int rate_in, int rate_out);

/* Opens `nslots` (>= 1) unconditioned slots, each an open stream of 0 samples (nhans_online_open_slots).  peak: finite,
 * >= 0.  flags: 0 or NHANS_LIVE_WET. */
int nhans_live_open_slots(nhans_ctx* ctx, int nslots, int rate_in, int in_format, double peak, int rate_out, int out_format,
                          double out_scale, int flags, void* stream, nhans_live** out);

/* Host only.  Slot `slot` becomes an open stream of 0 samples in all three stages, whatever it was; its conditioning
 * is kept (nhans_online_restart). */
int nhans_live_restart(nhans_live* obj, int slot);

/* The slot's conditioning, with the rules and the *first_frame_out of nhans_online_set_context /
 * nhans_online_set_embeddings (the context recordings are 16 kHz normalised float32).  The slot's streams keep running:
 * a join is nhans_live_restart + one of these, and one of these alone changes the conditioning of a running stream. */
int nhans_live_set_context(nhans_live* obj, int slot, const float* ctx_a_wav_dev, int64_t na, const float* ctx_b_wav_dev,
                           int64_t nb, void* stream, int64_t* first_frame_out);
int nhans_live_set_embeddings(nhans_live* obj, int slot, const float* emb_a_dev, const float* emb_b_dev, void* stream,
                              int64_t* first_frame_out);

/* Host only.  The wet factor w of the pushes that follow (finite; != 0 needs NHANS_LIVE_WET). */
int nhans_live_set_wet(nhans_live* obj, double wet);

/* Host only: the counts a push of in_counts_host[i] elements (end_host nullable) would report. */
int nhans_live_out_counts(const nhans_live* obj, const int64_t* in_counts_host, const int* end_host, int64_t* out_counts_host);

/* Appends in_offsets_host[i+1] - in_offsets_host[i] (>= 0) elements of in_dev (in_format) to slot i; end_host
 * (nullable) != 0 ends the slot's stream after them.  Writes the out_counts_host[i] samples that became final, as
 * out_format elements, at element out_offsets_host[i] of out_dev; the room out_offsets_host[i+1] - out_offsets_host[i]
 * must hold them (nhans_live_out_counts). */
int nhans_live_push(nhans_live* obj, const void* in_dev, const int64_t* in_offsets_host, const int* end_host, void* out_dev,
                    const int64_t* out_offsets_host, int64_t* out_counts_host, void* stream);

/* Look-ahead of a live slot.  (The two names do not begin with nhans_live_: the ten functions above are the whole set of
 * that prefix a binding of this section's first release checks for.)
 * nhans_lookahead_live_emitted: host only, no object -- the output contract above with the online stage at look-ahead L;
 * nhans_live_emitted is this function at L = 17.  Negative (NHANS_EINVAL) also for L outside 0..17.
 * nhans_lookahead_live_set: host only -- nhans_online_set_lookahead for the slot's online stage, allowed while the slot's
 * stream has 0 samples in all three stages (after open, or after nhans_live_restart), else NHANS_EINVAL and nothing
 * changes; L survives nhans_live_restart; the last push becomes final (nhans_live_rewind).  The output is then bit for
 * bit the offline chain above with nhans_enhance_clips under option "lookahead" = L. */
int64_t nhans_lookahead_live_emitted(int64_t nsamples, int ended, int rate_in, int rate_out, int lookahead);
int nhans_lookahead_live_set(nhans_live* obj, int slot, int lookahead);

/* Host only.  Undoes the most recent push in all three stages -- every stage wrote the half of its carried state that it
 * did not read -- so that it can be redone (nhans_online_rewind: a saturated push).  Once per push: a second rewind, one
 * before any push, or one after a restart / set call that followed the push, returns NHANS_EINVAL. */
int nhans_live_rewind(nhans_live* obj);

void nhans_live_close(nhans_live* obj);

/* ---- Conditioning captured from a slot's own stream -------------------------------------------------------------------
 * The set functions above take two 16 kHz, already normalised recordings that the caller owns.  A live caller has neither:
 * its audio is device-rate PCM, the 16 kHz version exists only inside the object, and the noise it wants removed is what
 * the microphone hears now -- the reference's own use is to record a piece of the environment and pass it as --neg
 * (its README.md).  The functions below condition slot i, side a or b, on the last NHANS_CAPTURE_SAMPLES samples slot i
 * itself has received, without a sample leaving the device.  Added without moving NHANS_ABI_VERSION; a caller that may meet
 * an older library looks them up by symbol.  (The names of the live pass-throughs begin with nhans_capture_, not with the
 * live prefix, whose set of names is closed.)
 *
 * Sample history.  nhans_capture_enable gives every slot a ring of NHANS_CAPTURE_SAMPLES floats (129 KB per slot, allocated
 * once; any time; idempotent; NHANS_ENOMEM and nothing changed if the allocation fails).  From then on every push also
 * copies each slot's new 16 kHz samples into its ring, sample k of the stream at position k mod NHANS_CAPTURE_SAMPLES
 * -- extra copy runs of the push's first launch (nhans_capture_plan), no launch more, and only the last
 * NHANS_CAPTURE_SAMPLES samples of a larger push.  Without the enable call a push is what it was, launch for launch.
 * The ring is not double-buffered as the carried state is.  The library keeps, per slot, vlo: the oldest sample of the
 * slot's current stream that the ring still holds -- N at enable time, 0 after nhans_online_restart, and after every push
 * max(vlo, N - NHANS_CAPTURE_SAMPLES), also when the push is then undone by nhans_online_rewind (its samples stay in the
 * ring, over older ones).  A capture needs N - NHANS_CAPTURE_SAMPLES >= vlo, else NHANS_ESHORT: too few samples yet, history
 * enabled too recently, or a rewound push not yet repeated (the message says which).  Repeating the rewound push with the
 * same input -- the redo of a saturated push -- makes the history valid again.
 *
 * Capture.  For entry k let x be the 16 kHz samples slot slots_host[k]'s stream has received and N their number.  The
 * context clip is x[N - NHANS_CAPTURE_SAMPLES : N] as stored; with NHANS_CAPTURE_NORMALISE it goes through the arithmetic of
 * nhans_peak_normalise with flags 0: float32(double(x) / (double(max|x|) + 1e-6)).  Row which_host[k] of the slot's embedding
 * pair becomes nhans_embed(nhans_stft_features(clip, max 200 frames)), BIT FOR BIT the row nhans_online_set_context would
 * store for that clip -- whatever the cutting of the stream into pushes, n, and the other entries of the call; the slot's
 * other row is untouched.  One gather kernel, ONE STFT and ONE tower pass over the n clips, then n row copies.
 * Semantics of the set functions: first_frame_out[k] (array nullable) receives R of entry k's slot, frames >= R use the
 * new row, the last push becomes final (nhans_online_rewind).  Ended streams may be captured (R = T; the rows serve the
 * slot's next stream, as conditioning survives a restart).  Capture does not make an unconditioned slot conditioned (such a
 * slot cannot have samples).  For a live object x is what the incoming converter handed on -- already divided by
 * peak + 1e-6 -- and N = nhans_resample_emitted(pushed, ended, rate_in, 16000); the converters keep running.
 * Errors (nothing changes, the function's name in nhans_last_error()): NHANS_EINVAL for history not enabled, n < 1, a slot
 * out of range, which not 0 or 1, a (slot, which) pair named twice, unknown flag bits, a NULL that is needed; NHANS_ESHORT as
 * above.  What the captured conditioning is worth is a property of the trained model; nothing in this library measures it. */
#define NHANS_CAPTURE_SAMPLES 32240   /* 199 * 160 + 400: the 200 context frames */
#define NHANS_CAPTURE_A 0
#define NHANS_CAPTURE_B 1
#define NHANS_CAPTURE_NORMALISE 1

/* Host only, no object.  The copy runs that append `count` samples to a ring that has seen n_before: runs_out[r] = {offset
 * in the push, ring position, length}, r < the returned number of runs (0 .. 2; 0 for count == 0).  The push uses this very
 * function.  Negative counts, or runs_out == NULL with count > 0: NHANS_EINVAL. */
int nhans_capture_plan(int64_t n_before, int64_t count, int64_t* runs_out /* [2][3] */);

int nhans_capture_enable(nhans_online* obj, void* stream);
int nhans_capture_context(nhans_online* obj, int n, const int* slots_host, const int* which_host, int flags, void* stream,
                          int64_t* first_frame_out /* [n], nullable */);
/* Copies the slot's current rows out ([512] floats each, either nullable): a learnt noise profile can be kept and handed
 * to nhans_online_set_embeddings elsewhere. */
int nhans_capture_embeddings(const nhans_online* obj, int slot, float* emb_a_out_dev, float* emb_b_out_dev, void* stream);

/* The same for the online stage of a live object.  The capture call makes the last live push final, as the live set
 * functions do; nhans_live_rewind and nhans_live_restart follow the vlo rules above. */
int nhans_capture_live_enable(nhans_live* obj, void* stream);
int nhans_capture_live_context(nhans_live* obj, int n, const int* slots_host, const int* which_host, int flags, void* stream,
                               int64_t* first_frame_out /* [n], nullable */);
int nhans_capture_live_embeddings(const nhans_live* obj, int slot, float* emb_a_out_dev, float* emb_b_out_dev, void* stream);

/* ---- Live sessions: level meter and automatic compensation --------------------------------------------------------------
 * The reference's --ac picks the wet factor itself: factor = snr_est / 20 with snr_est = mean(denoised^2) / mean(removed^2)
 * (SN/apply.py write_snc_outputs), three numpy lines once the whole file is known.  A live object has the 16 kHz denoised
 * and mixed pieces only on the device, so the functions below keep per-hop powers of each slot's 16 kHz output there and
 * derive from them a wet factor that follows that law over a trailing window -- applied inside the outgoing launch -- and
 * a meter the host can read.  Added without moving NHANS_ABI_VERSION; a caller that may meet an older library looks them up
 * by symbol.  (The names begin with nhans_level_: the live prefix's set of names is closed.)
 *
 * Definitions, for one slot.  d[n], m[n]: the final 16 kHz denoised and mixed samples of its stream, bit for bit those of
 * nhans_enhance_clips; r[n] = float32(m[n] - d[n]).  Hop h is samples [160 h, 160 h + 160).  A running stream's final
 * samples are a multiple of 320, so its hops are whole; an ended stream of T frames has 160 (T + 1) + 80 samples and its
 * last hop, of 80 samples, counts as a hop: nhans_level_hops(emitted, ended) hops are final.
 *   Powers (double; a product of two float32 is exact):  Pd[h] = sum double(d)^2, Pr[h] = sum double(r)^2,
 *     Pm[h] = sum double(m)^2, each hop summed by one wavefront in one fixed order (lane k: samples k, k + 64, k + 128,
 *     then the shuffle tree 32, 16, ... 1) whatever push made it final.
 *   Window sums, window W hops, 1 <= W <= 256:  Sd(h) = sum of Pd[j], j = max(h0, h - W + 1) ... h, ascending; Sr, Sm alike.
 *     W = 0: every hop since h0, a sequential running sum -- the reference's whole-file figure to date.  h0 is the first
 *     hop the state knows: 0 after open or nhans_live_restart, or the hop at which the meter was enabled.
 *   Gain of hop h:  g = (Sd / Sr) / 20 in double;  w_h = float32(min(max(g, 0), wmax));  w_h = 0 where Sr == 0 or g is NaN.
 *     The gain is constant over a hop and steps between hops; how large a step can be is the caller's choice of W.
 *   Mix:  sample n of hop h becomes c[n] = d + r * w_h, the three separately rounded float32 operations of step 1 of the
 *     live output arithmetic with w_h in place of the scalar, and the outgoing stream is the conversion of c, bit for bit.
 * Every figure depends on the recording (and on h0) only, never on how the stream was cut into pushes.
 *
 * Launches.  A push of an object whose meter was never enabled is launch for launch what it was.  With the meter enabled
 * a push that makes a hop final issues one launch more, "live_level", between the online stage and "live_out", one
 * workgroup per slot with new hops; a failure behind it puts every stage back as a failed live_out does.  The state is
 * double-buffered like the converters' carried samples: nhans_live_rewind is host-only here too.
 * What automatic compensation is worth is a property of the trained model; nothing in this library measures it. */

/* Host only, no object.  Final hops of a stream that has emitted `emitted` 16 kHz samples: emitted / 160, rounded up once
 * ended.  Negative (NHANS_EINVAL) for emitted < 0. */
int64_t nhans_level_hops(int64_t emitted, int ended);

/* Gives every slot its level state (6.3 KB per slot and half; idempotent).  Needs an object opened with NHANS_LIVE_WET,
 * else NHANS_EINVAL naming the flag.  h0 of a slot is the number of hops its stream has then; the last push becomes
 * final (nhans_live_rewind).  Pushes from now on also meter. */
int nhans_level_live_enable(nhans_live* obj, void* stream);

/* Host only.  window_hops 0 .. 256: the hops later pushes make final are mixed with their own w_h (window W = window_hops,
 * clamp wmax: finite, >= 0) instead of the factor of nhans_live_set_wet, which stays stored and can still be set;
 * the meter uses the same W and wmax (0 and 1.0 until the first such call).  window_hops -1: back to the stored fixed
 * factor from the next final hop on (wmax is checked and otherwise unused; the meter keeps its window).  Anything else,
 * or a meter not enabled: NHANS_EINVAL and nothing changes.  The last push becomes final (nhans_live_rewind). */
int nhans_level_live_auto(nhans_live* obj, int window_hops, double wmax);

/* The meter of a slot after its last final hop h: out[0..2] = Sd(h), Sr(h), Sm(h), out[3] = hops known (h + 1 - h0),
 * out[4] = w_h -- the law's gain, applied or not --, out[5] = snr_est = Sd / Sr (inf or NaN where Sr == 0), out[6..7] = 0.
 * One copy of 64 bytes and one synchronisation of the stream.  NHANS_ESHORT before the slot's first hop since h0. */
int nhans_level_live_read(nhans_live* obj, int slot, double* out_host /* [8] */, void* stream);

/* The gains w_h of the hops the last push made final for the slot, in hop order, to out_host (room for `cap`); returns
 * their number (out_host NULL: the number alone; 0 after a rewind or restart).  One copy, one synchronisation. */
int64_t nhans_level_live_gains(nhans_live* obj, int slot, float* out_host, int64_t cap, void* stream);

/* The whole-clip statement of the definitions, by the same kernel: clip i is samples [offsets_host[i], offsets_host[i+1])
 * of den_dev / mix_dev, an ended stream with h0 = 0 -- ceil(n / 160) hops, the last one as short as it is.  Writes one
 * gain per hop to w_out_dev, clip after clip, and (sums_out_dev nullable) the eight doubles of nhans_level_live_read
 * after each clip's last hop at sums_out_dev[8 i] (nothing for an empty clip).  window_hops 0 .. 256. */
int nhans_level_gains(nhans_ctx* ctx, const float* den_dev, const float* mix_dev, const int64_t* offsets_host, int nclips,
                      int window_hops, double wmax, float* w_out_dev, double* sums_out_dev, void* stream);

/* ---- Live sessions: interleaved multi-channel PCM in and out ------------------------------------------------------------
 * Capture and playback interfaces hand over interleaved frames -- element k * C + c is channel c of frame k --, almost
 * always stereo.  An object opened here is a nhans_live whose pushes take frames of channels_in channels and return frames
 * of channels_out channels (each 1 .. NHANS_INTERLEAVED_MAX_CHANNELS), formed and stored by the two converters' own
 * launches: no launch, buffer or copy is added, a push issues the launches of a mono object with as many slots doing the
 * same work.  Added without moving NHANS_ABI_VERSION; a caller that may meet an older library looks the functions up by
 * symbol.  (The names begin with nhans_interleaved_: the live prefix's set of names is closed.)
 *
 * NHANS_INTERLEAVED_DOWNMIX.  One slot per stream; channels_in and channels_out are independent.  Sample k of the slot's
 * incoming stream is
 *     x[k] = float32( (sum over c = 0 .. channels_in - 1 of double(s[k * channels_in + c])) / double(channels_in) ),
 * the sum starting at 0.0 and adding c in ascending order -- nhans_channel_mean's arithmetic, what the reference does to a
 * stereo file --, formed while the incoming converter stages its input, stored nowhere; the converter carries x.  Each
 * output sample, after steps 3 and 4 of the live output arithmetic, is stored channels_out times: dst[m * channels_out + c]
 * for every c.  The stream is bit for bit a mono float32 slot fed x.
 *
 * NHANS_INTERLEAVED_SPLIT.  channels_in == channels_out == C, and stream g owns the C consecutive slots g C .. g C + C - 1:
 * slot g C + c reads s[k * C + c] and writes dst[m * C + c], bit for bit a mono slot fed channel c alone, so every channel
 * is enhanced on its own and the stereo image survives.  Every per-slot function of a nhans_live -- restart, conditioning,
 * capture, look-ahead, the meter -- works on those slots as on any other; a caller gives the channels of a stream the same
 * conditioning or different ones.  Gains are NOT linked across the channels of a stream: the meter and the automatic wet
 * factor stay per slot, so automatic compensation may move two channels differently.
 * A push moves the C slots of a stream by the same frames with the same end flag, so they have to be in step: when a
 * push brings a stream frames or its end and its slots differ in samples taken, ended flag or look-ahead, the push is
 * refused with NHANS_EINVAL naming the stream and the slot that differs, and nothing changes -- after nhans_live_restart
 * of one channel alone, until the others are restarted too.
 *
 * Offsets and counts of the two functions below are per STREAM and in FRAMES; everything else -- the output contract
 * (nhans_live_emitted of the frames pushed), the arithmetic, rewind, the errors that change nothing -- is the live
 * section's.  nhans_live_push and nhans_live_out_counts refuse an object opened here, and the two functions below refuse
 * one opened with nhans_live_open_slots; each message names the function to call instead. */
#define NHANS_INTERLEAVED_DOWNMIX 0
#define NHANS_INTERLEAVED_SPLIT 1
#define NHANS_INTERLEAVED_MAX_CHANNELS 8

/* nhans_live_open_slots for `nstreams` (>= 1) streams of interleaved frames: nstreams slots (downmix) or nstreams *
 * channels_in slots (split), all unconditioned.  Channels outside 1 .. 8, split with channels_in != channels_out, an unknown
 * mode and everything nhans_live_open_slots refuses: NHANS_EINVAL.  Close with nhans_live_close. */
int nhans_interleaved_live_open(nhans_ctx* ctx, int nstreams, int channels_in, int channels_out, int mode, int rate_in,
                                int in_format, double peak, int rate_out, int out_format, double out_scale, int flags,
                                void* stream, nhans_live** out);

/* Host only: the frames a push of in_frames_host[g] frames (end_host nullable) would report per stream -- in split mode
 * the count all slots of the stream share; a stream whose slots are out of step is refused as the push refuses it. */
int nhans_interleaved_live_out_counts(const nhans_live* obj, const int64_t* in_frames_host, const int* end_host,
                                      int64_t* out_frames_host);

/* nhans_live_push in frames: stream g brings in_frame_offsets_host[g+1] - in_frame_offsets_host[g] (>= 0) frames that start
 * at element in_frame_offsets_host[g] * channels_in of in_dev; the out_frames_host[g] frames that became final are
 * written from element out_frame_offsets_host[g] * channels_out of out_dev on, and the room
 * out_frame_offsets_host[g+1] - out_frame_offsets_host[g], in frames, must hold them.  One call, the three stages of
 * nhans_live_push, its snapshots for a failed launch and for nhans_live_rewind; the runs of the slots of a split stream
 * point into the same frames, one channel apart. */
int nhans_interleaved_live_push(nhans_live* obj, const void* in_dev, const int64_t* in_frame_offsets_host, const int* end_host,
                                void* out_dev, const int64_t* out_frame_offsets_host, int64_t* out_frames_host, void* stream);

/* ---- Filterbank features of log-magnitude rows, offline and live ---------------------------------------------------------
 * Many consumers of the enhanced signal are machines -- speech, speaker and emotion recognisers -- that turn the waveform
 * straight back into 25 ms / 10 ms log-mel frames: the framing the network already works in (400-sample periodic Hann
 * window, hop 160, 201 bins 40 Hz apart).  The denoised log-magnitude row of frame g exists on the device the moment the
 * stack has run; the functions below turn such rows into filterbank features there, without the iSTFT, the outgoing
 * converter, a download and a second STFT.  Added without moving NHANS_ABI_VERSION; a caller that may meet an older
 * library looks them up by symbol.
 *
 * Definition.  A filterbank is n_out bands (1 .. NHANS_FBANK_MAX_OUT), a non-negative finite matrix W[n_out, 201] given in
 * double and stored as float32 (W32), power 1 or 2 and floor > 0 (stored as float32; it must be > 0 there).  For a row
 * x[201] (float32, natural log: what nhans_stft_features and nhans_mask_net write)
 *     p[k]   = exp(min(power * x[k], 88))                              float32 (expf)
 *     mel[m] = sum of W32[m, k] * p[k],  k ascending over band m's span   ONE chain of fmaf in float32 from +0.0f
 *     out[m] = ln(max(mel[m], floor))                                  float32 (logf)
 * where the span of a band reaches from its first to its last non-zero float32 weight (a band without one is empty:
 * out[m] = ln(floor)).  Over the domain of the network's rows, x in [ln 1e-5 - 20, 16], every p is a normal float32 for
 * both powers and the clamp at 88 changes nothing; outside it the clamp keeps p finite.  A row's bits depend on the row and
 * the filterbank only -- never on where the row sits in a call, which call computed it, or how a stream was cut into pushes.
 * The spans of all bands together may hold NHANS_FBANK_MAX_SPAN entries (a mel bank of 128 bands has about 400): a matrix
 * over that is refused, the message naming the cap.
 * What the features are worth to a recogniser is a property of the trained model; nothing in this library measures it. */
#define NHANS_FBANK_MAX_OUT 128
#define NHANS_FBANK_MAX_SPAN 8192
#define NHANS_FBANK_HTK 0           /* mel = 2595 log10(1 + f / 700) */
#define NHANS_FBANK_SLANEY 1        /* mel = f / (200/3) below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27) from 1 kHz on */
#define NHANS_FBANK_NORM_NONE 0
#define NHANS_FBANK_NORM_SLANEY 1   /* band m times 2 / (p[m+2] - p[m]) */
#define NHANS_FBANK_MIXED 1         /* attach flag: also the features of the same frames' unprocessed rows (plane 1) */

typedef struct nhans_fbank nhans_fbank;

/* Host only, no object.  The usual triangular matrix, in double: p[0 .. n_out + 1] equally spaced on the mel scale `scale`
 * between f_min and f_max (0 <= f_min < f_max <= 8000 Hz), bin k at f_k = 40 k Hz,
 *     W[m, k] = max(0, min((f_k - p[m]) / (p[m+1] - p[m]), (p[m+2] - f_k) / (p[m+2] - p[m+1])))   times the norm's factor
 * -- the definitions librosa and torchaudio use.  Writes W to w_out_host ([n_out * 201], nullable) and returns the number
 * of bands that are empty after float32 rounding (>= 0: narrow bands between two bins), or NHANS_EINVAL (n_out, the
 * frequencies, an unknown scale or norm) with nothing written. */
int nhans_fbank_design(int n_out, double f_min, double f_max, int scale, int norm, double* w_out_host);

/* A filterbank on ctx's device.  The matrix is checked first, before anything touches a device: n_out outside 1 .. 128,
 * power other than 1 or 2, a floor that is not finite and > 0 as a float32, a weight that is negative, NaN, infinite or
 * beyond float32, or spans over NHANS_FBANK_MAX_SPAN are NHANS_EINVAL and *out is NULL.  The table is on the device when
 * the call returns. */
int nhans_fbank_open(nhans_ctx* ctx, const double* w_host, int n_out, int power, double floor, void* stream, nhans_fbank** out);
void nhans_fbank_close(nhans_fbank* fb);

/* Any [nrows, 201] log-magnitude rows -> [nrows, n_out] features: the denoised_out_dev of nhans_mask_net, or the logmag of
 * nhans_stft_features for the unprocessed signal.  One launch, "fbank_rows"; nrows == 0 launches nothing.  The call uses
 * the context the filterbank was opened on and is ordered with that context's other calls. */
int nhans_fbank_rows(nhans_fbank* fb, const float* logmag_dev, int64_t nrows, float* out_dev, void* stream);

/* Features of a live stream.  Attach COPIES fb's table into the object (one small allocation and a synchronous copy, no
 * launch), so fb may be closed afterwards; fb == NULL detaches (flags must then be 0).  Allowed between pushes; it applies
 * from the next push on and voids the rows of the last one.  With a filterbank attached, a push that computes frames --
 * frames [R_old, R_new) of the "Look-ahead" contract, per slot -- issues ONE launch more, "online_fbank", behind the stack:
 * it reads the push's denoised rows (plane 0) and, with NHANS_FBANK_MIXED, the same frames' unprocessed centre rows
 * (plane 1) and writes a buffer of the object, which grows on demand by at least doubling.  The rows are bit for bit
 * nhans_fbank_rows of nhans_mask_net's denoised_out_dev (option "lookahead" = the slot's L) and of nhans_stft_features'
 * logmag for the same samples.  An object with nothing attached issues exactly the launches it issued before.
 * Frame g is centred on sample 160 g + 200 of the slot's 16 kHz stream and its features exist 10 L + 25 ms after that
 * sample arrived: no later than the audio, and usually a hop earlier (the even-pair rule does not apply to them). */
int nhans_fbank_online_attach(nhans_online* obj, nhans_fbank* fb, int flags);

/* Copies the rows the MOST RECENT push computed for `slot` (plane 0: denoised, 1: mixed -- NHANS_EINVAL unless attached with
 * NHANS_FBANK_MIXED) to out_dev ([rows, n_out], room for cap_rows rows) on `stream` and returns their number;
 * out_dev == NULL only returns the number.  *first_frame_out (nullable) is the stream frame index of the first row -- with
 * no rows, of the next frame the slot will compute.  The number is 0 for a slot that computed nothing in the last push, and
 * for every slot after nhans_online_rewind, an attach, a restart of that slot or a push whose launches were refused, until
 * the next push; the redo of a rewound push brings the redone rows.  Negative on error: nothing attached, a slot or plane
 * out of range, cap_rows too small. */
int64_t nhans_fbank_online_read(nhans_online* obj, int slot, int plane, float* out_dev, int64_t cap_rows,
                                int64_t* first_frame_out, void* stream);

/* The same for the online stage of a live object, mono or interleaved; in split mode a channel is its slot.  The frames are
 * those of the slot's 16 kHz stream, after the incoming converter and the fixed peak. */
int nhans_fbank_live_attach(nhans_live* obj, nhans_fbank* fb, int flags);
int64_t nhans_fbank_live_read(nhans_live* obj, int slot, int plane, float* out_dev, int64_t cap_rows, int64_t* first_frame_out,
                              void* stream);

/* ---- Live sessions: full-band output, the band above 8 kHz carried through ------------------------------------------------
 * Everything a live object returns has been through the 16 kHz network path: at 44.1 or 48 kHz the output carries nothing
 * above 8 kHz.  A full-band object adds the input's own high band, delayed to line up with the output, inside the
 * outgoing launch.  It applies to an object with rate_in == rate_out == r, r one of 22050, 24000, 32000, 44100, 48000,
 * 88200 or 96000, opened with NHANS_LIVE_WET, mono or interleaved.  Per slot, with
 *   x[n]  the slot's incoming sample n as float32, as the incoming stage forms it (the PCM sample; with interleaved frames
 *         the downmix mean or the slot's own channel),
 *   u[n]  = float32(double(x[n]) / (peak + 1e-6)) -- the incoming stage's division --, 0 from the end of the input on,
 *   d[k], m[k]  the final 16 kHz denoised and mixed-round-trip samples, c[k] the combined one (d + (m - d) * w with the
 *         fixed or the hop's automatic factor; d where the factor is 0),
 *   g     the slot's high-band gain, float32, 0 <= g <= 4,
 * the outgoing stage converts e[k] = c[k] - g * m[k] where it converted c[k] (same filter, tap order and carried samples,
 * which now are e), lo[n] being its output n, and stores y[n] = lo[n] + g * u[n] through the arithmetic it stored lo[n]
 * through: float32(double(y) * out_scale), then the rounding and the clamp for int16.  Each of the two expressions is a
 * product and a sum rounded separately in float32.  In real numbers y = R(c) + g (u - R(m)), R the conversion 16 kHz ->
 * r: u - R(m) is the input less its own trip through 16 kHz, the complement of the two cascaded low-passes -- below
 * 6 kHz what is left of a tone is the filters' pass-band ripple, at most 2.3e-3 of it (about -53 dB, times g), from
 * 8.5 kHz on it is the tone.  Output sample n is aligned with input sample n.
 *   g = 0: the output of an object that never enabled the feature, bit for bit.
 *   wet = 1, g = 1, int16 in and out on the scale it came in on (out_scale == peak + 1e-6): the input itself, delayed.
 *   A changed gain is piecewise: e[k] takes the gain of the push that brought 16 kHz sample k into the outgoing stage,
 *   g * u[n] that of the push that emits n.
 * The input samples that have no output yet are kept per slot in a double-buffered hold of H(r) float32 samples, H(r) the
 * largest N - nhans_lookahead_live_emitted(N, 0, r, r, L) over N and L <= 17; a push of an enabled object issues one small
 * launch more ("live_hold" in the profile) and still one "live_out".  Rewind and restart stay host-only. */
/* H(r), in samples; NHANS_EINVAL for a rate that is not one of the seven. */
int64_t nhans_fullband_hold_samples(int rate);
/* Enables the full band of every slot with gain 1.0 (idempotent); the push before it cannot be rewound.  NHANS_EINVAL,
 * with nothing changed: rate_in != rate_out; a rate <= 16000; an object opened without NHANS_LIVE_WET; a slot that has
 * taken a sample (enable after open, or after restarting every slot that has). */
int nhans_fullband_live_enable(nhans_live* obj, void* stream);
/* The gain of `slot` (-1: of every slot), finite, 0 <= gain <= 4, from the next push on; the push before it cannot be
 * rewound.  In downmix mode the high band is that of the downmix, copied to every output channel. */
int nhans_fullband_live_set_gain(nhans_live* obj, int slot, double gain);
/* The whole-clip twin, the kernels of ended streams: nclips clips of x at `rate` (x_format int16 or float32, clip i at
 * x_offsets[i] .. x_offsets[i + 1]) with their d and m at 16 kHz (clip i at offsets16[i] .. offsets16[i + 1] of both) ->
 * y as out_format, nhans_resample_out_count(n16, 16000, rate) samples per clip from out_offsets[i] on.  in_denom is the
 * divisor of u (peak + 1e-6); wet the fixed factor, or wet_hops_dev (nullable) one factor per hop of 160 samples of each
 * clip, ceil(n16 / 160) per clip one clip after the other -- the layout of nhans_level_gains. */
int nhans_fullband_mix(nhans_ctx* ctx, const void* x_dev, int x_format, const int64_t* x_offsets_host, const float* den_dev,
                       const float* mix_dev, const int64_t* offsets16_host, int nclips, int rate, double in_denom, double wet,
                       const float* wet_hops_dev, double gain, double out_scale, int out_format, void* out_dev,
                       const int64_t* out_offsets_host, void* stream);

/* ---- Scoring against a clean target -----------------------------------------------------------------------------------
 * How good an output is, computed where the output is: SI-SDR, SNR, segmental SNR of waveforms, and the reference's
 * training loss and the log-spectral distance of log-magnitude rows, in double, without a sample leaving the device.  Added
 * without moving NHANS_ABI_VERSION; a caller that may meet an older library looks the functions up by symbol.
 *
 * Waveform figures of an estimate e and a target t (float32, n = min(ne, nt) common samples; every operation in double):
 *   See = sum e^2, Stt = sum t^2, Set = sum e t, Sdd = sum (e - t)^2
 *   snr_db    = 10 log10(Stt / Sdd)
 *   alpha     = Set / Stt,  r = fma(-alpha, t, e),  Srr = sum r^2  (a second pass over the samples, not the expanded form)
 *   si_sdr_db = 10 log10(alpha alpha Stt / Srr);  e bit-equal to t: alpha == 1, Srr == 0, +inf
 *   segsnr_db = mean over the frames f < nhans_num_frames(n) with Pt != 0 of clamp(10 log10(Pt / Pd), -10, 35), Pt and Pd the
 *               sums of t^2 and (e - t)^2 over samples [160 f, 160 f + 400); Pd == 0 scores 35; a frame with Pt == 0 is
 *               skipped and counted in frames_skipped
 *   Edges follow IEEE and are not refused: Stt == 0 (n == 0 included) gives alpha = 0 and NaN for both dB figures, no
 *   counted frame gives NaN for segsnr_db, non-finite samples propagate.
 * Row figures of two [frames, 201] float32 log-magnitude tensors E and T (any rows of the library: the denoised rows of
 * nhans_mask_net, or nhans_stft_features of two waveforms), d = E - T in double:
 *   loss   = mean over frames of (sum_k d^2 imp[k]) / 201, imp = float32 linspace(2, 1, 201): the reference's training loss
 *   lsd_db = mean over frames of sqrt((sum_k ((20 / ln 10) d)^2) / 201)
 *   no frame: NaN for both.
 * Every figure is a function of the clip pair alone: the order of each sum is fixed relative to the clip's first sample
 * (n-hans_amd/csrc/score.hip states it), so a record has the same bits alone or in any batch, at any offset, on every run.
 *
 * Clip i of the estimates is est_dev[est_offsets_host[i] .. est_offsets_host[i + 1]), of the targets likewise with its own
 * offsets.  out_dev receives NHANS_SCORE_FIELDS doubles per clip, frames_out_dev (nullable) one row of three doubles per
 * frame, clip after clip, nhans_num_frames(n_i) rows for clip i: the waveform call writes column 0 (the frame's clamped
 * value, NaN where the frame was skipped), the row call columns 1 and 2 (the frame's loss and lsd); each leaves the
 * other's columns untouched.  NHANS_EINVAL, naming the clip, before anything is launched: nclips < 0, a NULL that is
 * needed, an offset array that descends. */
#define NHANS_SCORE_FIELDS 16   /* n, See, Stt, Set, Sdd, alpha, Srr, snr_db, si_sdr_db, segsnr_db,
                                   frames_counted, frames_skipped, 0, 0, 0, 0 */
#define NHANS_SCORE_ROW_FIELDS 8 /* frames, loss, lsd_db, 0 ... */
int nhans_score_wave(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                     const int64_t* tgt_offsets_host, int nclips, double* out_dev, double* frames_out_dev, void* stream);
/* Clip i's rows are rows frame_offsets_host[i] .. frame_offsets_host[i + 1] of both tensors. */
int nhans_score_rows(nhans_ctx* ctx, const float* est_rows_dev, const float* tgt_rows_dev, const int64_t* frame_offsets_host,
                     int nclips, double* out_dev, double* frames_out_dev, void* stream);

/* Mixing at a chosen SNR on the device: the rule of the reference's demo and evaluation readers (n-hans_amd/mixing.py:
 * domixing, domixing_separator), bit for bit, so that a corpus can be mixed, enhanced and scored without its audio
 * leaving HBM (n-hans_amd/csrc/mix.hip).  Inputs are float32 and finite: a speech clip s of
 * n >= 1 samples, a noise a to KEEP and a noise b to DROP of ma, mb >= 1 samples, and an SNR for each.
 *   fit      A[i] = a[i mod ma] where ma < n, else a[i], for i < n; B likewise
 *   power    sq[i] = float32(x[i] x[i]); S = ((0.0 + double(sq[0])) + double(sq[1])) + ..., one dependent chain of float64
 *            additions in index order (the chain is part of the definition); P = S / double(n)
 *   gain     f = nhans_mix_snr_factor(snr_db) = pow(10.0, -snr_db / 10.0), the C library's on the HOST;
 *            g = sqrt((P_s / P_noise) f) in double, 1 where P_noise == 0; g32 = float32(g)
 *   raw      raw[i] = (s[i] + g32a A[i]) + g32b B[i]: two float32 products and two float32 sums, each rounded on its own;
 *            without a keep noise (index -1: the separator's two-way mix) raw[i] = s[i] + g32b B[i]
 *   finish   pk = max |raw|, p = float32(pk + 1e-6f), mixture[i] = raw[i] / p;
 *            unit = float32(float32(pk / p) + 1e-6f): the peak of the normalised mixture plus 1e-6;
 *            target = (s + g32a A) / unit, keep = g32a A / unit, drop = g32b B / unit -- divided by about 1, not by p: the
 *            reference's quirk.  Without a keep noise target = s / unit and keep is zeros.
 *   record   NHANS_MIX_FIELDS doubles: P_s, P_keep, P_drop, g_keep, g_drop, pk, unit, 0 (P_keep = 0 and g_keep = 1 without
 *            a keep noise)
 *   An all-zero mixture gives p = 1e-6f and zeros, P_s == 0 the gain 0; non-finite samples: unspecified.
 * Speech clip i is speech_dev[speech_offsets_host[i] .. [i + 1]), noise clip i likewise in its own buffer.  Job j mixes
 * speech clip speech_idx_host[j] with the noises keep_idx_host[j] (-1: none; a NULL array: none for every job) and
 * drop_idx_host[j] at snr_keep_host[j] and snr_drop_host[j] dB, so that one triple serves many SNR pairs; its outputs
 * are elements out_offsets_host[j] .. [j + 1] of every output buffer, which must hold its n samples.  target_dev,
 * keep_dev, drop_dev and records_dev are nullable.  A power is computed once per distinct (clip, fitted length) of a
 * call.  NHANS_EINVAL, naming the job, before anything is launched: njobs < 0, a NULL that is needed, an index out of
 * range, a speech or noise clip of no samples, outputs too short. */
#define NHANS_MIX_FIELDS 8
/* (host only; an int with an output argument like every other call of this header that can refuse) */
int nhans_mix_snr_factor(double snr_db, double* factor_out);
int nhans_mix(nhans_ctx* ctx, const float* speech_dev, const int64_t* speech_offsets_host, int nspeech, const float* noise_dev,
              const int64_t* noise_offsets_host, int nnoise, const int* speech_idx_host, const int* keep_idx_host,
              const int* drop_idx_host, const double* snr_keep_host, const double* snr_drop_host, int njobs, float* mixture_dev,
              float* target_dev, float* keep_dev, float* drop_dev, const int64_t* out_offsets_host, double* records_dev,
              void* stream);

/* ---- STOI and extended STOI against a clean target ----------------------------------------------------------------------
 * The intelligibility figures of Taal et al. (2011) and Jensen & Taal (2016), computed where the signals are
 * (n-hans_amd/csrc/stoi.hip).  Added without moving NHANS_ABI_VERSION; a caller that may meet an
 * older library looks the functions up by symbol.  x is the target and y the estimate, both float32 at 10 kHz (not the
 * network's 16 kHz: nhans_stoi_resample below), n = min(nx, ny) common samples; every operation is in double.
 *   window    w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)), i < 256: the 256 inner points of a 258-point symmetric Hann window
 *             (Matlab's hanning(256))
 *   framing   M0 = ceil((n - 256) / 128) frames for n > 256, else 0; frame m is samples [128 m, 128 m + 256).  A final frame
 *             that would end exactly at n is not taken (the published code's rule).
 *   silence   P_m = sum (w x_m)^2, P_max = max P_m; frame m is kept iff P_m > P_max * 1e-4 (40 dB; the product rounded
 *             once).  The decision is taken on the target and applied to both signals; Mk frames are kept, none where
 *             P_max == 0.
 *   rejoining the kept windowed frames of each signal are overlap-added at hop 128 in their kept order (a signal of
 *             128 (Mk - 1) + 256 samples) and framed again by the same rule: Mf = Mk - 1 frames (0 for Mk <= 1), each
 *             windowed by w again, zero-padded to 512 and transformed.
 *   bands     X[j][q] = sqrt(sum_{k in [lo_j, hi_j)} |X_q(k)|^2), 15 third-octave bands from 150 Hz, [lo, hi) =
 *             (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109) (109,138)
 *             (138,174) (174,219): the nearest bins of linspace(0, 10000, 513) to 150 * 2^(j/3) * 2^(-+1/6)
 *   stoi      S = Mf - 29 segments for Mf >= 30, else 0; segment s is columns s ... s + 29.  Per band: a = |x| / (|y| + eps),
 *             y' = min(a y, (1 + 10^(15/20)) x); x and y' are made zero-mean over the 30 columns and divided by their norm
 *             + eps; d_s = (sum_j sum_q x^ y'^) / 15; stoi = mean_s d_s; eps = 2^-52
 *   estoi     per segment and signal each row (band) is made zero-mean and divided by its norm + eps, then each column
 *             likewise; e_s = (sum x~ y~) / 30; estoi = mean_s e_s
 *   edges     S == 0 (a clip too short, or everything silent) gives NaN for both figures, the counts filled in -- IEEE, as the
 *             scoring section above, where the published Python package returns 1e-5 with a warning.  Non-finite samples:
 *             unspecified.
 *   record    NHANS_STOI_FIELDS doubles: n, frames (M0), frames_kept (Mk), segments (S), stoi, estoi, 0, 0
 * Every figure is a function of the clip pair alone: the order of each sum is fixed relative to the clip's first sample
 * (stoi.hip states it), there are no floating-point atomics, and a record has the same bits alone or in any batch, at any
 * offset, on every run.
 *
 * Clip i of the estimates is est10_dev[est_offsets_host[i] .. est_offsets_host[i + 1]), of the targets likewise with its own
 * offsets.  out_dev receives NHANS_STOI_FIELDS doubles per clip.  segments_out_dev (nullable) receives rows of two doubles
 * d_s, e_s, clip after clip: how many segments a clip has is known on the device only, so clip i's rows begin at row
 * sum_{k < i} max(0, M0_k - 30) -- room for the segments of a clip without a silent frame -- and its first `segments` rows
 * are written.  NHANS_EINVAL, naming the clip, before anything is launched: nclips < 0, a NULL that is needed, an offset
 * array that descends.
 *
 * nhans_stoi_resample brings 16 kHz float32 clips to 10 kHz: the filter design, float32 taps and single fmaf chain of
 * nhans_resample for L = 5, M = 8 (half = 80), on the same kernel -- a pair for this purpose only, not one of
 * nhans_resample's.  Clip i gives nhans_stoi_out_count(n_i) = ceil(5 n_i / 8) samples from out_offsets_host[i] on and is
 * refused where the room is less.  The published STOI implementations convert with another filter (Matlab's resample
 * design): figures computed from 16 kHz signals are this library's, not theirs. */
#define NHANS_STOI_FIELDS 8     /* n, frames, frames_kept, segments, stoi, estoi, 0, 0 */
int64_t nhans_stoi_out_count(int64_t n16);      /* host only */
int nhans_stoi_resample(nhans_ctx* ctx, const float* in16_dev, const int64_t* in_offsets_host, int nclips, float* out10_dev,
                        const int64_t* out_offsets_host, void* stream);
int nhans_stoi(nhans_ctx* ctx, const float* est10_dev, const int64_t* est_offsets_host, const float* tgt10_dev,
               const int64_t* tgt_offsets_host, int nclips, double* out_dev, double* segments_out_dev, void* stream);

/* ---- BSS Eval: SDR, SIR and SAR against target and interferer ---------------------------------------------------------------
 * The decomposition of Vincent, Gribonval and Fevotte (2006; bss_eval_sources of the published toolboxes) of one estimate
 * with fixed roles, computed where the signals are (n-hans_amd/csrc/bsseval.hip).  Added without
 * moving NHANS_ABI_VERSION; a caller that may meet an older library looks the function up by symbol.  Inputs are float32:
 * an estimate e and J = 1 or 2 sources, s_0 the target and s_1 the interferer, every signal cut to the n samples all of
 * them have, and a filter length L, 1 <= L <= 512.  Every signal is zero outside [0, n), t runs over [0, n + L - 1), and
 * every operation is in double.
 *   correlations  r_jk[d] = sum_t s_j[t] s_k[t + d] for |d| < L;  q_k[b] = sum_t e[t + b] s_k[t] for 0 <= b < L.  A product of
 *                 two float32 values is exact in double; the sums are formed directly, in a fixed order (bsseval.hip).
 *   Gram system   G[(j,a),(k,b)] = r_jk[a - b], J L x J L, symmetric, block Toeplitz;  D[(k,b)] = q_k[b].
 *   solves        G C = D by Cholesky (lower factor, no pivoting) and two triangular solves; the leading L x L block of G
 *                 with D[:L] likewise gives C0 (its factor is the leading block of G's factor: one factorisation serves both).
 *                 A pivot that is not finite or is <= J L 2^-52 G_kk (G_kk the diagonal element of G in the pivot's row)
 *                 makes the clip SINGULAR: the six energies and the three figures are NaN, the flag field is 1, n, J and L
 *                 are filled in, and the filters, where asked for, are NaN.  An all-zero source is singular, and so is a
 *                 clip of no samples.  Nothing is refused for it.
 *   projections   P[t] = sum_k sum_b C[k,b] s_k[t - b];  s_target[t] = sum_b C0[b] s_0[t - b];  e_interf = P - s_target;
 *                 e_artif = e - P.
 *   energies      each one fixed-order sum of squares over t: E_e = |e|^2, E_tgt = |s_target|^2, E_int = |e_interf|^2,
 *                 E_art = |e_artif|^2, E_dist = |e - s_target|^2, E_ti = |s_target + e_interf|^2
 *   figures       sdr_db = 10 log10(E_tgt / E_dist), sir_db = 10 log10(E_tgt / E_int), sar_db = 10 log10(E_ti / E_art), by
 *                 IEEE.  With J = 1 e_interf is identically zero: sir_db = +inf and sar_db has the value of sdr_db.
 *                 Non-finite samples: unspecified.
 *   record        NHANS_BSS_FIELDS doubles: n, J, L, E_e, E_tgt, E_int, E_art, E_dist, E_ti, sdr_db, sir_db, sar_db, singular,
 *                 0, 0, 0
 * The decomposition does not change when a source is scaled or filtered by up to L taps.  The published toolboxes form
 * the correlations by FFT and fall back to least squares on a singular Gram matrix; figures agree with theirs to rounding
 * at best, not bit for bit.  Every figure is a function of the clip tuple and L alone: it has the same bits alone or in
 * any batch, at any offset, on every run; no floating-point atomics, no reduction whose shape depends on the batch.
 *
 * Clip i of the estimates is est_dev[est_offsets_host[i] .. est_offsets_host[i + 1]); src_dev is a HOST array of nsrc device
 * pointers and src_offsets_host a host array of nsrc offset arrays: clip i of source j is src_dev[j][src_offsets_host[j][i]
 * .. [i + 1]).  out_dev receives NHANS_BSS_FIELDS doubles per clip.  filters_out_dev (nullable) receives per clip C -- J L
 * doubles, source 0's taps first -- and then C0 -- L doubles.  The factor of G takes (J L)^2 doubles of the workspace per
 * clip, 8 MiB at J = 2 and L = 512: the clips of a call are worked in groups whose factors together stay within 2 GiB
 * (256 clips at full size; option "bss_group_bytes"), and the grouping changes no bit of any record.  NHANS_EINVAL, naming
 * the clip, before anything is launched: nclips < 0, nsrc not 1 or 2, filt_len outside 1 ... 512, a NULL that is needed,
 * an offset array that descends, a clip of more than 2^31 - 1 samples. */
#define NHANS_BSS_FIELDS 16     /* n, J, L, E_e, E_tgt, E_int, E_art, E_dist, E_ti, sdr_db, sir_db, sar_db, singular, 0, 0, 0 */
int nhans_bss_eval(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* const* src_dev,
                   const int64_t* const* src_offsets_host, int nsrc, int nclips, int filt_len, double* out_dev,
                   double* filters_out_dev, void* stream);

/* ---- Delay estimation: scoring signals that are not aligned -----------------------------------------------------------------
 * Every scoring call above pairs sample u of the estimate with sample u of the target.  Where the target comes from outside
 * -- another microphone, a loop-back capture, another front end with a delay of its own -- the pair is aligned first, where
 * the signals are (n-hans_amd/csrc/align.hip).  Added without moving NHANS_ABI_VERSION; a caller that
 * may meet an older library looks the functions up by symbol.  Inputs per clip are an estimate e of ne samples and a target
 * t of nt samples, both float32 and finite, and one max_lag = D per call, 0 <= D <= 16000 (one second at 16 kHz).  Every
 * operation is in double.
 *   correlation   for -D <= d <= D:  c[d] = sum_u e[u + d] t[u] over u in [max(0, -d), min(nt, ne - d)); an empty range gives
 *                 +0.0.  d > 0 means the estimate is LATE: e[u + d] lines up with t[u].  A product of two float32 values is
 *                 exact in double; the sum is formed directly, in a fixed order (align.hip states it).
 *   delay         the d with the largest c[d].  The comparison is signed: an estimate of inverted polarity is not searched
 *                 for (its largest c[d] is wherever the signals happen to agree best in sign).  Of equal values the one
 *                 with the smaller |d| wins, and of -d and +d the non-negative one.  All-zero input therefore gives 0.
 *   confidence    rho = c[delay] / sqrt(See Stt), See = sum e^2 and Stt = sum t^2 over the WHOLE clips, each a fixed-order sum
 *                 (the product rounded once, then the root, then the quotient).  IEEE applies: 0 / 0 is NaN, and nothing is
 *                 refused for it.
 *   common count  n_common = max(0, min(ne - max(delay, 0), nt - max(-delay, 0))): the samples the cut pair has.
 *   record        NHANS_ALIGN_FIELDS doubles: ne, nt, D, delay, c_peak, rho, n_common, 0
 * Whole samples only: no sub-sample delay, no polarity search, no clock drift (one delay per clip).  c[d] is a function of
 * the clip pair and of d alone: it has the same bits for every D >= |d|, alone or in any batch, at any offset of either
 * buffer, beside any neighbours, on every run -- no floating-point atomics, no reduction whose shape depends on the batch or
 * on D: the sample tiles are anchored at the target's u = 0 and a clip's tile parts are added in ascending order.  Only
 * samples inside a clip are ever fetched.  Non-finite samples: unspecified.
 *
 * Clip i of the estimates is est_dev[est_offsets_host[i] .. est_offsets_host[i + 1]), of the targets likewise with its own
 * offsets.  out_dev receives NHANS_ALIGN_FIELDS doubles per clip.  corr_out_dev (nullable) receives the 2 max_lag + 1 values
 * c[-D] ... c[D] per clip, lag -D first.  The workspace holds nclips (2 max_lag + 1) doubles when corr_out_dev is NULL and
 * otherwise only a table of the clips.  NHANS_EINVAL, naming the clip, before anything is launched and with nothing written:
 * nclips < 0, max_lag outside 0 ... 16000, a NULL that is needed, an offset array that descends, a clip of more than
 * 2^31 - 1 samples.
 *
 * nhans_align_common(ne, nt, delay) is n_common (host only).
 *
 * nhans_align_cut writes, for clip i with d = delay_host[i], e[max(d, 0) .. + n_common) to est_out_dev and t[max(-d, 0) ..
 * + n_common) to tgt_out_dev, both from element out_offsets_host[i] on: one launch for the whole call.  The cut pairs are
 * what the scoring calls above take, with out_offsets_host for both signals.  Either signal may be left out: est_dev and
 * est_out_dev both NULL, or tgt_dev and tgt_out_dev both NULL -- the offsets of a signal left out still say how long it is.
 * A further signal that is sample-aligned with the target (the interferer of nhans_bss_eval) is cut by a second call
 * with that signal in the target's place, the same delays and no estimate.  NHANS_EINVAL, naming the clip, before anything is
 * launched and with nothing written: nclips < 0, a NULL that is needed (one of a pair alone included), an offset array that
 * descends, a delay d > ne or -d > nt (more than the clip it shortens), an output room shorter than n_common. */
#define NHANS_ALIGN_FIELDS 8    /* ne, nt, D, delay, c_peak, rho, n_common, 0 */
#define NHANS_ALIGN_MAX_LAG 16000
int nhans_align(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                const int64_t* tgt_offsets_host, int nclips, int max_lag, double* out_dev, double* corr_out_dev, void* stream);
int64_t nhans_align_common(int64_t ne, int64_t nt, int64_t delay);      /* host only */
int nhans_align_cut(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                    const int64_t* tgt_offsets_host, int nclips, const int64_t* delay_host, float* est_out_dev, float* tgt_out_dev,
                    const int64_t* out_offsets_host, void* stream);

/* ---- LLR, cepstral distance and frequency-weighted segmental SNR against a clean target --------------------------------------
 * How much an enhancement distorted the speech itself: three figures of the objective-measure set of Hu & Loizou (2008;
 * Quackenbush et al. 1988), computed where the signals are (n-hans_amd/csrc/quality.hip).  Added
 * without moving NHANS_ABI_VERSION; a caller that may meet an older library looks the functions up by symbol.  e is the
 * estimate and t the target, both float32 at 16 kHz, scored over the common prefix n = min(ne, nt) and converted to double
 * once.  Every operation below is in double and is one IEEE operation rounded to nearest: x * y, x + y, x - y, x / y,
 * fma(x, y, z) = x y + z rounded once, sqrt.  Nothing is left to contraction.  "chain over i" means acc = +0.0, then one
 * operation per i, ascending.
 *   framing   N = 480, hop 120; M = 0 for n < 480, else (n - 480) / 120 + 1 (integer division); frame f is samples
 *             [120 f, 120 f + 480).  w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 481), computed on the host in double
 *             (nhans_quality_tables returns the very table).  xw[i] = x[120 f + i] * w[i].
 *   LPC       order P = 16, per frame and signal.  r[k], k = 0 ... 16: the chain over i = 0 ... 479 - k of
 *             acc = fma(xw[i], xw[i + k], acc).  Levinson-Durbin: E = r[0], a[0] = 1; for m = 1 ... 16:
 *                 acc = r[m]; for j = 1 ... m - 1 ascending: acc = fma(a[j], r[m - j], acc);   k_m = -(acc / E);
 *                 for j = 1 ... m - 1: a'[j] = fma(k_m, a[m - j], a[j]);   then a[j] = a'[j], a[m] = k_m;
 *                 E = E * fma(-k_m, k_m, 1)          (this is E_m)
 *   LLR       q(a) = the chain over i = 0 ... 16 of acc = fma(a[i], row_i, acc), row_i the chain over j = 0 ... 16 of
 *             acc = fma(r_t[|i - j|], a[j], acc): always on the TARGET's autocorrelation.  num = q(a_e), den = q(a_t),
 *             llr_f = min(max(ln(num / den), 0), 2).
 *   CD        c[m], m = 1 ... 16: s = the chain over k = 1 ... m - 1 of acc = fma(((double)k / (double)m) * c[k], a[m - k], acc);
 *             c[m] = (-a[m]) - s.  dc2 = the chain over m = 1 ... 16 of acc = fma(d, d, acc), d = c_t[m] - c_e[m].
 *             cd_f = min(max((10 / ln 10) * sqrt(2 * dc2), 0), 10), 10 / ln 10 = 4.342944819032518.
 *   skipped   a frame has no LLR and no CD (its values are NaN; it is counted out of frames_lpc) where r_t[0] == 0 or
 *             r_e[0] == 0, an E_m of either recursion is not a positive finite number (the recursion stops there), or den
 *             or num is not a positive finite number.
 *   fwSegSNR  each windowed frame is zero-padded to 512 and transformed by the radix-8 transform of
 *             n-hans_amd/csrc/fft512.h (one transform per signal: an all-zero frame has an all-zero spectrum, exactly);
 *             |X_k| of the target's and |Y_k| of the estimate's, k = 0 ... 256, |u| = sqrt(fma(u_i, u_i, u_r * u_r)).  Band matrix W:
 *             [K][257], K <= 32, non-negative; the default has K = 25 triangles on the HTK mel scale between 0 and 8000 Hz
 *             over the bin frequencies 31.25 k (the construction of nhans_fbank_design on 257 bins; nhans_quality_tables
 *             returns it).  X_j = the chain over k = 0 ... 256 of acc = fma(W[j][k], |X_k|, acc); Y_j likewise.
 *             s_j = 35 where X_j == Y_j, else min(max(10 * log10((X_j * X_j) / ((X_j - Y_j) * (X_j - Y_j))), -10), 35);
 *             g_j = pow(X_j, 0.2); G = the chain over j of acc = acc + g_j, D = the chain over j of acc = fma(g_j, 35 - s_j, acc);
 *             fw_f = 35 - D / G: the weighted mean sum_j g_j s_j / sum_j g_j, formed from the bands' deficits so that equal
 *             signals give 35 exactly.  A frame with G == 0 is skipped (NaN; counted out of frames_fw).
 *   figures   llr, cd_db, fwsegsnr_db: the chain acc = acc + v_f over the kept frames, f ascending, divided by their count.
 *             llr_95, cd_95_db: the mean of the q = (19 Mk + 10) / 20 (integer division) smallest of the Mk kept values --
 *             the published practice of dropping the worst 5 % of the frames.  The q-th smallest value v is found exactly
 *             (a radix select on the bit patterns, which order as the non-negative values do; no sort); the figure is
 *             (b + (double)(q - nb) * v) / (double)q, b the chain acc = acc + v_f over the nb kept frames with v_f < v, f
 *             ascending.  No kept frame: NaN, the counts filled in (the convention of nhans_stoi).  ln, log10 and pow are
 *             the device library's (a few units in the last place); non-finite samples: unspecified.
 *   record    NHANS_QUALITY_FIELDS doubles: n, frames (M), frames_lpc, frames_fw, llr, llr_95, cd_db, cd_95_db,
 *             fwsegsnr_db, then zeros.  Lower is better for LLR and CD, higher for fwSegSNR.
 * The band table is this library's own.  The published MATLAB code of the measure set uses a fixed table of 25 critical
 * bands with Gaussian-shaped filters and a 1,024-point transform; it was not at hand, and nothing here claims equal
 * figures with it.  Not computed: weighted spectral slope, Itakura-Saito, PESQ and the composites CSIG / CBAK / COVL (they
 * need PESQ); other sample rates; live sessions.
 * Every figure is a function of the clip pair (and W) alone: no floating-point atomics, no reduction whose shape depends
 * on the batch; a record and every per-frame value have the same bits alone or in any batch, at any offset, on every run.
 * Only samples inside a clip are fetched.
 *
 * Clip i of the estimates is est_dev[est_offsets_host[i] .. est_offsets_host[i + 1]), of the targets likewise with its own
 * offsets.  bands_host (nullable: the default matrix) is a HOST array of nbands * 257 doubles, nbands ignored where it is
 * NULL.  out_dev receives NHANS_QUALITY_FIELDS doubles per clip.  frames_out_dev (nullable) receives rows of three doubles
 * llr_f, cd_f, fw_f, clip after clip: clip i's M_i rows begin at row sum_{k < i} M_k; NaN where the frame was skipped.  The
 * workspace holds three doubles a frame when frames_out_dev is NULL.  NHANS_EINVAL, naming the clip, before anything is
 * launched and with nothing written: nclips < 0, nbands outside 1 ... 32 or a weight that is negative or not finite, a
 * NULL that is needed, an offset array that descends, a clip of more than 2^31 - 1 samples.
 *
 * nhans_quality_lpc (for tests and diagnosis) runs the LPC launch alone and writes NHANS_QUALITY_LPC_FIELDS doubles per
 * frame, rows as above: r_t[0 .. 16], r_e[0 .. 16], a_t[0 .. 16], a_e[0 .. 16], num, den, dc2, 0.  Where a recursion stopped
 * its a[1 .. 16] are NaN, and so is what is computed from them.
 * nhans_quality_tables (host only) copies the 480 doubles of w and the 25 * 257 of the default W; either may be NULL. */
#define NHANS_QUALITY_FIELDS 16 /* n, frames, frames_lpc, frames_fw, llr, llr_95, cd_db, cd_95_db, fwsegsnr_db, 0 ... */
#define NHANS_QUALITY_LPC_FIELDS 72
#define NHANS_QUALITY_BINS 257
#define NHANS_QUALITY_BANDS 25
#define NHANS_QUALITY_MAX_BANDS 32
int nhans_quality(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                  const int64_t* tgt_offsets_host, int nclips, const double* bands_host, int nbands, double* out_dev,
                  double* frames_out_dev, void* stream);
int nhans_quality_lpc(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                      const int64_t* tgt_offsets_host, int nclips, double* lpc_out_dev, void* stream);
int nhans_quality_tables(double* window_out, double* bands_out);        /* host only */

/* ---- Drift-aware alignment: the delay tracked over a clip and warped out ----------------------------------------------------
 * nhans_align estimates one whole-sample delay per clip.  Where estimate and target were sampled by two clocks -- a far
 * microphone, a loop-back capture through a sound card -- the delay is neither an integer nor constant: converters differ by
 * tens to a few hundred ppm, and 100 ppm move a 10 s clip by 16 samples.  These calls track the delay over the clip, fit a
 * line to it and resample the estimate onto the target's clock (n-hans_amd/csrc/drift.hip).  Added
 * without moving NHANS_ABI_VERSION; a caller that may meet an older library looks the functions up by symbol.
 *   model      target sample u lines up with position p(u) = a + u + b u of the estimate: a is the delay at u = 0 in samples,
 *              real-valued (a > 0: the estimate is late, the convention of nhans_align), b the drift (b > 0: the estimate's
 *              clock runs fast), |b| <= 2^-10 (977 ppm), |a| <= 2^31.  All arithmetic is in double, one IEEE operation rounded
 *              to nearest each (nothing is contracted); "chain" means acc = +0.0, then acc = fma(x, y, acc) per index,
 *              ascending.  Inputs are float32 at any rate.  A sample outside a clip is a zero and is never fetched.
 *   table      T = 16, Q = 512.  G[q][k] = sinc(x) kaiser(x / T; beta = 10), x = k - q / Q, for q = 0 ... Q and k = -T + 1 ... T:
 *              sinc(x) = sin(pi x) / (pi x), kaiser(r; beta) = I0(beta sqrt(1 - r^2)) / I0(beta), designed on the host in double;
 *              row 0 is set to the exact unit impulse.  D[q][k] = G[q + 1][k] - G[q][k], q < Q, rounded once.  The
 *              interpolator is flat within 2e-5 up to 0.39 of the sample rate (6.3 kHz at 16 kHz), where its transition
 *              band begins: content above that is attenuated and images.  nhans_drift_table (host only) copies the
 *              (Q + 1) 2T doubles of G and the Q 2T of D, tap k at column k + T - 1; either pointer may be NULL.
 *   segments   blocks of B = 4096 target samples at hop H = 2048: a clip of nt samples has J = 0 for nt < B, else
 *              (nt - B) / H + 1 (integer division) -- nhans_drift_segments (host only); samples after the last full block are
 *              not used.  Each call takes a centre line (ca, cb) per clip and one search radius R, 1 <= R <= 1024.  Segment
 *              j's centre lag is z_j = floor(fma(cb, j H + (B - 1) / 2, ca) + 0.5), computed on the host.
 *   lag vector c_j[d] = sum_i e[j H + i + d] t[j H + i] over i = 0 ... B - 1, for d in [z_j - R - T, z_j + R + T]: two tiles of
 *              2048 samples anchored at the block's first sample, each one chain (the products are exact), the second
 *              tile's part added to the first's.  c_j[d] is a function of the pair, of j and of d alone.
 *   integer    d* = the d of [z_j - R, z_j + R] with the largest c_j[d]; of equal values the one with the smaller |d - z_j|,
 *   peak       and of z_j - r and z_j + r the latter (the order of nhans_align, taken relative to z_j).
 *   fine peak  v_k = the lag vector interpolated at d* + k / 32, k = -32 ... 32: with w = floor(k / 32) and r = k - 32 w, the chain
 *              over the taps i = -T + 1 ... T of fma(c_j[d* + w + i], G[16 r][i], acc); a lag outside the vector (only d* + 17 at
 *              k = 32 can be; its weight is exactly 0) is passed over.  The best k: the larger value, then the smaller |k|,
 *              then the larger k.  For |k| < 32, den = (v_{k-1} - 2 v_k) + v_{k+1}; where den < 0 the parabola's offset is
 *              delta = ((v_{k-1} - v_{k+1}) / (2 den)) / 32, clamped to -1/64 ... 1/64; otherwise and for |k| = 32, delta = 0.
 *              tau_j = (d* + k / 32) + delta.
 *   abscissa   E_t = sum t[j H + i]^2 and N = sum i t[j H + i]^2 over the block, each in a fixed order (drift.hip states it);
 *              u_j = j H + N / E_t: the block's energy centroid, not its centre -- the delay a block measures is the delay
 *              where its energy is.
 *   confidence E_e = sum e[j H + i + d*]^2 over the block; rho_j = v_k / sqrt(E_e E_t) (the product rounded once, the root, the
 *              quotient).  IEEE applies: a silent block gives NaN for u_j and rho_j, and nothing is refused for it.
 *   flags      1: the peak is at the edge of the search, d* = z_j - R, d* = z_j + R, k = -32 or k = 32;  2: E_t == 0 or E_e == 0.
 *   record     NHANS_DRIFT_FIELDS doubles per segment: u_j, tau_j, rho_j, E_t, v_k, d*, flags, z_j.
 *   line fit   nhans_drift_fit (host only), from the records of one clip, rho_min (0.3 is the Python default) and trim (1.0):
 *              the valid segments have flags == 0 and rho >= rho_min.  Weighted least squares of tau on u with weights
 *              w = E_t, every sum over the segments ascending from +0.0, every product rounded by itself:
 *              W = sum w, mu = (sum w u) / W, mt = (sum w tau) / W, Suu = sum (w du) du, Sut = sum (w du) dt with du = u - mu and
 *              dt = tau - mt; b = Sut / Suu, a = mt - b mu.  One trimming pass: the segments with |tau - (a + b u)| > trim are
 *              dropped and, if any was, the rest is fitted again.  rms_residual = sqrt((sum (w r) r) / W) over the segments
 *              used, r the residual to the final line.  out: NHANS_DRIFT_FIT_FIELDS doubles a, b, n_valid, n_used,
 *              rms_residual, fit_ok.  fit_ok = 0 where fewer than 3 segments were used, where W or Suu is not positive (then
 *              a, b and the residual are NaN) or where |b| > 2^-10.
 *   warp       for clip i with (a, b) and a target of nt samples, the output covers the maximal range [u_lo, u_hi) of [0, nt)
 *              with 0 <= p(u) <= ne - 1 -- nhans_drift_range (host only), computed with the device's own expression of p;
 *              an empty range is 0, 0.  p = fma(b, u, a) + u (two roundings), m = floor(p), f = (p - m) Q (exact),
 *              q = min(floor(f), Q - 1), lambda = f - q, g_k = fma(lambda, D[q][k], G[q][k]), and
 *              y[u] = (float) the chain over k = -T + 1 ... T of fma(e[m + k], g_k, acc).  With a an integer and b = 0 the output
 *              is e[a + u] bit for bit (row 0 is the unit impulse; a sample -0.0 comes out as +0.0).  The aligned target is
 *              t[u_lo .. u_hi), and a further signal that is sample-aligned with the target is cut likewise: nhans_align_cut
 *              with no estimate, estimate lengths u_hi - u_lo and delay -u_lo.
 * Out of scope: a drift that is not linear over the clip (a clock that wanders, a dropped buffer), a polarity search, and
 * live sessions.  Every record and every output sample has the same bits alone or in any batch, at any offset of either
 * buffer, beside any neighbours, for every R that reaches the same lags, on every run: no floating-point atomics, no
 * reduction whose shape depends on the batch.  Only samples inside a clip are fetched.  Non-finite samples: unspecified.
 *
 * nhans_drift_track: clip i of the estimates is est_dev[est_offsets_host[i] .. est_offsets_host[i + 1]), of the targets
 * likewise with its own offsets; centre_a_host and centre_b_host hold one line per clip.  out_dev receives
 * NHANS_DRIFT_FIELDS doubles per segment, clip after clip: clip i's J_i records begin at record sum_{k < i} J_k.
 * corr_out_dev (nullable) receives the 2 (R + T) + 1 values of every segment's lag vector, lag z_j - R - T first, in the same
 * order.  The workspace holds a table of the segments only.  NHANS_EINVAL, naming the clip, before anything is launched
 * and with nothing written: nclips < 0, radius outside 1 ... 1024, a NULL that is needed, an offset array that descends, a
 * clip of more than 2^31 - 1 samples, a line that is not finite, |cb| > 2^-10, |ca| > 2^31 or a centre whose lags
 * z_j - R - T ... z_j + R + T leave the int32 range.
 *
 * nhans_drift_warp: the estimates as above; tgt_offsets_host says how long the targets are (their samples are not
 * read); a_host and b_host hold one line per clip.  Clip i's u_hi - u_lo samples are written from out_dev[out_offsets_host[i]]
 * on: one launch for the whole call.  NHANS_EINVAL, naming the clip, before anything is launched and with nothing written:
 * nclips < 0, a NULL that is needed, an offset array that descends, a clip of more than 2^31 - 1 samples, a line that is
 * not finite, |b| > 2^-10, |a| > 2^31, an output room shorter than the range. */
#define NHANS_DRIFT_FIELDS 8    /* u, tau, rho, E_t, v_peak, d_int, flags, z */
#define NHANS_DRIFT_FIT_FIELDS 6 /* a, b, n_valid, n_used, rms_residual, fit_ok */
#define NHANS_DRIFT_TAPS 16
#define NHANS_DRIFT_PHASES 512
#define NHANS_DRIFT_BLOCK 4096
#define NHANS_DRIFT_HOP 2048
#define NHANS_DRIFT_MAX_RADIUS 1024
int nhans_drift_table(double* g_out, double* d_out);                    /* host only */
int64_t nhans_drift_segments(int64_t nt);                               /* host only */
int nhans_drift_range(int64_t ne, int64_t nt, double a, double b, int64_t* u_lo_out, int64_t* u_hi_out);    /* host only */
int nhans_drift_fit(const double* records_host, int nsegments, double rho_min, double trim, double* out_host);  /* host only */
int nhans_drift_track(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const float* tgt_dev,
                      const int64_t* tgt_offsets_host, int nclips, const double* centre_a_host, const double* centre_b_host,
                      int radius, double* out_dev, double* corr_out_dev, void* stream);
int nhans_drift_warp(nhans_ctx* ctx, const float* est_dev, const int64_t* est_offsets_host, const int64_t* tgt_offsets_host,
                     int nclips, const double* a_host, const double* b_host, float* out_dev, const int64_t* out_offsets_host,
                     void* stream);

/* ---- Phase refinement: Griffin-Lim iterations after the mask ---------------------------------------------------------
 * The enhanced waveform has always been rebuilt from the network's log-magnitudes and the MIXTURE's phase.  These calls
 * move that phase towards one that is consistent with the magnitudes, on the device, without a waveform reaching HBM
 * between the inverse and the forward transform (n-hans_amd/csrc/phase.hip; the same definition
 * in float64: n-hans_amd/phase.py).  Added without moving NHANS_ABI_VERSION; a caller that may meet an older library
 * looks the functions up by symbol.
 *
 * A clip has T >= 1 frames of 201 bins; lm are its log-magnitude rows, A = exp(lm) with nhans_istft's exp, rounded to
 * float32.  The state t is complex float32 [T, 201], stored as (re, im) pairs.
 *   u(z)       z / |z|, and 1 + 0j where |z| is zero or below the smallest normal float32 (1.18e-38) -- the convention
 *              atan2(0, 0) = 0 of nhans_stft_features.  On the device: z times a power of two that brings it into range
 *              (2^64 below 2^-40, 2^-68 above 2^40), m = re^2 + im^2, r = the hardware reciprocal square root of m
 *              refined once (r (1.5 - 0.5 m r^2)), u = (re r, im r).  Non-finite z: unspecified.
 *   P(lm, t)   c = A u(t) (c = 0 for frames outside the clip).  x = inverse 400-point transform, synthesis window and
 *              overlap-add of c exactly as nhans_istft defines them: the imaginary parts of bins 0 and 200 are dropped,
 *              two frames share one complex transform, every sample is the sum over its <= 3 frames in ascending order.
 *              d = analysis window and forward real-input transform of the frames of x exactly as nhans_stft_features
 *              defines them before its log and angle.  d is complex float32 [T, 201].
 *   iteration  t_0 = cos ph + i sin ph from the input phases (nhans_istft's sine and cosine).  d_n = P(lm, t_n), then
 *              t_{n+1} = fma(alpha, d_n - d_{n-1}, d_n) per component with d_{-1} := d_0 (so t_1 = d_0).
 *   result     after N iterations phase_out = angle(t_N) with nhans_stft_features' atan2.  N = 0 copies the input phases
 *              bit for bit.  The final waveform is nhans_istft(lm, phase_out).
 *   inc[n]     sum (|d_n| - A)^2 / sum A^2 over the clip, n = 0 ... N - 1: the relative inconsistency.  |d| is the float32
 *              square root of re^2 + im^2, the difference is taken in float32, squares and sums are double.  The order is
 *              fixed: a frame's 201 terms with bins ascending (fma chain), then over the frames of the clip lane l of 64
 *              sums frames l, l + 64, ... ascending and the 64 sums go through the tree 32, ..., 1 of the scoring kernels.
 *              NaN where sum A^2 is zero.
 * There is no log, atan2, sine or cosine inside an iteration: exp(lm) is taken once per call into a plane of its own
 * and only the last state is turned into angles.  The clip edges are not perfect-reconstruction regions of the window
 * pair, so P is not idempotent there and inc need not fall monotonically.
 * Every output has the same bits for a clip alone or in any batch, at any position, on every run.  Inputs are only read;
 * nothing is written outside the outputs.  The workspace holds the A plane, two state planes (three with momentum) and the
 * frame partials: 20 (28) bytes per bin.
 *
 * nhans_phase_project: one projection.  t_dev and d_out_dev are complex rows [F, 201] (F = frame_offsets_host[nclips]);
 *   inc_out_dev (nullable) receives one double per clip.
 * nhans_phase_refine: N = iters iterations (0 <= iters <= 256) with momentum alpha (0 <= alpha < 1; 0 is plain
 *   Griffin-Lim and the recommended value: 0.99 lowers inc faster and loses SI-SDR after about 8 iterations).
 *   phase_out_dev [F, 201] may be phase_in_dev itself.  inc_out_dev (nullable) receives double [nclips][iters].
 * NHANS_EINVAL before anything is launched and with nothing written: a NULL that is needed, nclips < 0, iters or alpha
 * outside their range, offsets that descend, a clip without a frame or with more than 5,000,000 (the message names it).
 *
 * Option "phase_iters" (default 0, 0 ... 256) and nhans_phase_set_alpha (default 0.0): with N > 0 nhans_enhance_clips
 * refines the denoised rows from the mixture's phase between the mask net and the iSTFT of denoised_wav_dev -- bit for
 * bit nhans_istft over nhans_phase_refine of the denoised rows and the phase_out_dev tap.  The mixed_wav round trip and
 * all taps stay as they are (phase_out_dev is the MIXTURE's phase).  With N = 0 the call issues exactly the launches it
 * always has.  Online and live objects ignore the option: every iteration reaches two frames further into the future
 * (frame f of d_n depends on frames f - 2 ... f + 2 of t_n), so N iterations would add 2 N frames = 20 N ms of latency
 * to a stream whose whole look-ahead is 17 frames.
 * What the iterations are worth on a trained model's rows is unmeasured here (no trained weights ship with the library);
 * on the clean target's own magnitudes with the mixture's phase they gain 1.4 - 3.7 dB SI-SDR (README). */
#define NHANS_PHASE_MAX_ITERS 256
int nhans_phase_set_alpha(nhans_ctx* ctx, double alpha);
int nhans_phase_project(nhans_ctx* ctx, const float* logmag_dev, const float* t_dev, const int64_t* frame_offsets_host, int nclips,
                        float* d_out_dev, double* inc_out_dev, void* stream);
int nhans_phase_refine(nhans_ctx* ctx, const float* logmag_dev, const float* phase_in_dev, const int64_t* frame_offsets_host,
                       int nclips, int iters, double alpha, float* phase_out_dev, double* inc_out_dev, void* stream);

/* ---- Mask-driven MVDR beamforming of multi-channel clips ---------------------------------------------------------------
 * A multi-channel clip has always been reduced to the mean of its channels (nhans_channel_mean) before anything else.
 * These calls use what an array carries, the phase differences between its microphones: a mask (the network's, or any)
 * picks out the spatial covariance of speech and of noise, and a distortionless linear filter (MVDR, Souden's form) is put
 * on the channels.  n-hans_amd/csrc/mvdr.hip; the same definition in float64:
 * n-hans_amd/mvdr.py.  Added without moving NHANS_ABI_VERSION; a caller that may meet an older library looks the functions
 * up by symbol.
 *
 * A clip has C channels, 1 <= C <= 8, of n samples each and T = nhans_num_frames(n) >= 1 frames.  C is one value per call.
 *   planes     clip i is C planes of n_i samples one after the other: channel c begins at planes + C off[i] + c n_i, with
 *              off = sample_offsets_host counted in samples PER CHANNEL (the offsets the mono calls take for one channel).
 *   X          the spectra, complex float32 stored as (re, im), in the planes' layout: the T_i rows of 201 bins of
 *              channel c of clip i begin at row C foff[i] + c T_i, foff[i] = sum_{j<i} T_j -- the rows nhans_stft_features
 *              gives for the planes taken as nclips * C clips.  X_c[t, k] is what nhans_stft_features holds before its log
 *              and angle: logmag_out_dev and phase_out_dev of nhans_mvdr_spectra (nullable, [C F, 201] in X's layout, F =
 *              foff[nclips]) are the analysis kernel's log and atan2 of the very registers X is stored from, and equal
 *              nhans_stft_features' rows of the channel-clips bit for bit.
 *   mask       float32 rows [F, 201] at foff.  m = min(max(v, 0), 1), where max(NaN, 0) = 0: a NaN counts as 0 (the bin of
 *              that frame is all noise).  With NHANS_MVDR_LOGGAIN the rows are a log-gain g -- what nhans_mask_net writes
 *              to logits_out_dev -- and v = 1 for g > 0, else exp(g) with nhans_istft's exp; a NaN g counts as m = 0.
 *   Phi        per clip and bin, in double, x = (X_0 ... X_{C-1})[t, k]:  Phi_s = sum_t m x x^H,  Phi_n = sum_t (1 - m) x x^H
 *              with 1 - m formed in double.  Entry (i, j) of a frame is p = x_i conj(x_j), each part one rounding (the two
 *              products of float32 values are exact in double), then fma(m, p, sum) and fma(1 - m, p, sum).  The diagonal's
 *              imaginary part is 0.  The sum runs over the frames in ASCENDING order, one chain per entry: the kernel
 *              splits a bin's entries, not its frames, over the waves of a workgroup, so an entry has one owner and no
 *              partial sums are combined.  Every value is a function of the clip alone.
 *              cov_out_dev (nullable): complex double [nclips][2][C][C][201] -- Phi_s then Phi_n, entry (i, j), bin last.
 *   w          tr = sum_i Re Phi_n[i][i] (i ascending);  Phi_n' = Phi_n + loading (tr / C) I, 0 <= loading <= 1 (1e-6 is the
 *              recommended value);  Phi_n' = L L^H by Cholesky, column by column, in double;  G = Phi_n'^-1 Phi_s by the two
 *              triangular solves, a column at a time;  tau = sum_j Re G[j][j] (j ascending);  w = G[:, ref] / tau.  No
 *              steering vector and no eigen-decomposition; w does not change when either mask's sum is scaled.
 *              FALLBACK, w = e_ref (the reference channel passes through) and the bin counts in fallback_bins: tr = 0; a
 *              pivot that is not positive and finite; tau not positive and finite; a part of w not finite.  A mask of all
 *              ones or all zeros therefore returns the reference channel and says so.
 *              w_out_dev: complex double [nclips][201][C].
 *   y          y[t, k] = sum_c conj(w_c) X_c[t, k], channels ascending, four fma per channel in double, rounded ONCE to
 *              complex float32.  The output is rows [F, 201] at foff: lm = log(max(|y|, 1e-5)) and ph = atan2(im, re) with
 *              the analysis kernel's square root, log and atan2 (note the max: the analysis rows add 1e-5 instead).
 *              loggain_dev (nullable, rows [F, 201]): lm + g in float32 -- nhans_mask_net's own last step.
 *              y_out_dev of nhans_mvdr_apply (nullable): y itself, complex float32 [F, 201], before any log-gain.  The
 *              beamformed signal is thus what every other signal here is: nhans_mask_net, nhans_istft, nhans_phase_refine,
 *              nhans_fbank_rows and nhans_score_rows take the rows as they are.
 *   record     NHANS_MVDR_FIELDS = 6 doubles per clip: frames, channels, ref, fallback_bins, energy_ref = sum |X_ref|^2,
 *              energy_out = sum |y|^2 of the float32 y (before any log-gain).  energy_ref: per bin over the frames
 *              ascending, then lane l of 64 sums bins l, l + 64, l + 128, l + 192 ascending and the 64 sums go through the
 *              tree 32, ..., 1 of the scoring kernels.  energy_out: per frame a lane's bins l, l + 64, ... ascending and
 *              the tree; then over the frames lane l sums frames l, l + 64, ... ascending and the tree.
 *              nhans_mvdr_weights writes fields 0 ... 4 and NaN into energy_out; nhans_mvdr_apply writes energy_out alone
 *              (records_dev nullable).  nhans_mvdr writes all six.
 * Non-finite samples: the bins they reach fall back or not as the rules above say; their rows are unspecified.
 * Every output has the same bits for a clip alone or in any batch, at any position, on every run, and through nhans_mvdr
 * as through the three stage calls.  Inputs are only read; nothing is written outside the outputs.
 * Launches: spectra 1 ("mvdr_spectra"), weights 2 ("mvdr_cov", "mvdr_solve"), filter 1 ("mvdr_apply") and with a record
 * one more ("mvdr_energy").  nhans_mvdr keeps X (8 C bytes per bin and frame), the covariances and, unless asked for, w
 * in the workspace.
 * NHANS_EINVAL before anything is launched and with nothing written, the message naming the clip where there is one:
 * nchannels outside 1 ... 8, ref outside 0 ... nchannels - 1, loading outside [0, 1] (or NaN), unknown flag bits, a NULL that
 * is needed, nclips < 0, offsets that descend, a clip without a frame or with more than 5,000,000. */
#define NHANS_MVDR_MAX_CHANNELS 8
#define NHANS_MVDR_FIELDS 6
#define NHANS_MVDR_LOGGAIN 1
int nhans_mvdr_spectra(nhans_ctx* ctx, const float* planes_dev, const int64_t* sample_offsets_host, int nclips, int nchannels,
                       float* x_out_dev, float* logmag_out_dev, float* phase_out_dev, void* stream);
int nhans_mvdr_weights(nhans_ctx* ctx, const float* x_dev, const float* mask_dev, const int64_t* frame_offsets_host, int nclips,
                       int nchannels, int ref, double loading, int flags, double* w_out_dev, double* cov_out_dev,
                       double* records_out_dev, void* stream);
int nhans_mvdr_apply(nhans_ctx* ctx, const float* x_dev, const double* w_dev, const float* loggain_dev,
                     const int64_t* frame_offsets_host, int nclips, int nchannels, float* logmag_out_dev, float* phase_out_dev,
                     float* y_out_dev, double* records_dev, void* stream);
int nhans_mvdr(nhans_ctx* ctx, const float* planes_dev, const int64_t* sample_offsets_host, int nclips, int nchannels,
               const float* mask_dev, int ref, double loading, int flags, const float* loggain_dev, float* logmag_out_dev,
               float* phase_out_dev, double* w_out_dev, double* records_out_dev, void* stream);

/* Profiling (option "profile" = 1): per-kernel launch counts, summed milliseconds, summed
 * algorithmic FLOPs / bytes ("flops": 2*M*K*N of the DIRECT convolution whichever form runs it) and the
 * FLOPs the matrix cores executed for them ("mfma_flops": three products per MAC in split-f16 mode, fewer
 * MACs for the Winograd form) since the last reset, as a JSON object written to buf.  Synchronises
 * the recorded events.  Returns the number of bytes needed (excluding the NUL). */
int nhans_profile_json(nhans_ctx* ctx, char* buf, size_t buflen);
int nhans_profile_reset(nhans_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* NHANS_HIP_H */
