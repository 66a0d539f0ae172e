/* pk_synth.h -- C ABI of libpk_synth.so, the MI355X (gfx950) synthesis engine
 * behind Parakeet's inference API.
 *
 * The reference (PaddlePaddle/Parakeet) is pure Python over Paddle ops; it has
 * no FFI of its own.  The seam this ABI replaces is the Python class API of
 * the synthesis path; each entry point names the reference method whose device
 * work it performs (paths relative to the reference repository root):
 *
 *   pk_pwg_*    parakeet/models/parallel_wavegan/parallel_wavegan.py
 *               PWGGenerator.__init__ :369-443, set_state_dict,
 *               remove_weight_norm :485-496, inference :498-520 (forward :445-472),
 *               PWGInference.forward :772-775
 *   pk_fs2_*    parakeet/models/fastspeech2/fastspeech2.py
 *               FastSpeech2.__init__ :52-296, inference :468-558
 *               (_forward(is_inference=True) :377-466),
 *               FastSpeech2Inference.forward :668-671
 *   pk_wf_*     parakeet/models/waveflow.py ConditionalWaveFlow.infer :785-805, forward :759-782
 *   pk_tts_*    parakeet/models/transformer_tts/transformer_tts.py TransformerTTS.inference :511-647,
 *               TransformerTTSInference.forward :757-767
 *   pk_taco_*   parakeet/models/tacotron2.py Tacotron2.infer :781-840 (Tacotron2Decoder.infer :474-541),
 *               Tacotron2.forward :691-778 (Tacotron2Decoder.forward :419-472)
 *   pk_spk_*    parakeet/models/lstm_speaker_encoder.py LSTMSpeakerEncoder.embed_sequences / embed_utterance :40-53,
 *               similarity_matrix :55-104 and the softmax loss :122-134 (pk_spk_ge2e; the EER :136-145 is host code)
 *   pk_stft_mel parakeet/modules/audio.py STFT.magnitude :202-215 + MelScale :226-229,
 *               parakeet/data/get_feats.py LogMelFBank.get_log_mel_fbank :80-88
 *
 * Conventions
 *   - Every function returns PK_OK (0) or a negative pk_status; the message of
 *     the last failure on the calling thread is pk_last_error().  Nothing
 *     aborts.  The Python shim maps the codes back to the exception classes the
 *     reference raises (ValueError / AssertionError / NotImplementedError).
 *   - Plain pointers and sizes only.  Parameter arrays handed to *_set_param are
 *     HOST pointers and are copied (the caller may free them at once, like
 *     set_state_dict).  Data pointers of the compute calls are DEVICE pointers
 *     unless the call's `flags` has PK_HOST_IO, in which case they are host
 *     pointers and the engine stages them (synchronous on return).
 *   - A pk_ctx owns one HIP device + one stream.  Handles created on a context
 *     are not thread-safe; different contexts may be used concurrently.  Calls
 *     are asynchronous on the context's stream unless stated; use pk_sync().
 *   - Batches are "packed ragged": utterance b owns rows [cu[b], cu[b+1]) of a
 *     row-major array; lengths are given per utterance on the host.
 */
#ifndef PK_SYNTH_H
#define PK_SYNTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PK_OK = 0,
    PK_EINVAL = -1,        /* bad argument value              -> ValueError          */
    PK_ESHAPE = -2,        /* shape / size mismatch           -> AssertionError      */
    PK_EUNSUPPORTED = -3,  /* configuration not implemented   -> NotImplementedError */
    PK_EHIP = -4,          /* HIP runtime failure             -> RuntimeError        */
    PK_ENOMEM = -5,        /* allocation failure              -> MemoryError         */
    PK_ESTATE = -6         /* call order (e.g. not finalized) -> RuntimeError        */
} pk_status;

enum {
    PK_HOST_IO = 1,            /* flags bit: data pointers are host memory */
    PK_PWG_C_HAS_CONTEXT = 2,  /* pk_pwg_infer: mel rows already carry aux_context_window frames on both
                                  sides of every utterance (PWGGenerator.forward); default: the engine
                                  replicate-pads (PWGGenerator.inference) */
    PK_APPLY_NORMALIZER = 4,   /* pk_fs2_decode / pk_ss_decode / pk_pwg_infer: apply the ZScore registered with
                                  pk_*_set_normalizer in THIS call (the *Inference wrappers of the reference:
                                  FastSpeech2Inference.forward fastspeech2.py:668-671, PWGInference.forward
                                  parallel_wavegan.py:772-775, SpeedySpeechInference.forward :221-231).
                                  Without it the call stays in the model's own (normalised) domain, as
                                  model.inference() does in the reference -- the registered statistics are
                                  per-handle state, their use is per call */
    PK_TTS_KEEP_ATT = 8        /* pk_tts_infer: keep the encoder-decoder attention weights (TransformerTTS.inference's
                                  third return value) for pk_tts_read */
};

typedef struct pk_ctx pk_ctx;
typedef struct pk_pwg pk_pwg;
typedef struct pk_fs2 pk_fs2;
typedef struct pk_wf pk_wf;
typedef struct pk_mel pk_mel;

/* ---------------------------------------------------------------- context */
const char* pk_last_error(void);
const char* pk_version(void);
/* Create a context on HIP device `device_id` with its own stream. */
int pk_ctx_create(int device_id, pk_ctx** out);
/* Run on an externally owned hipStream_t (e.g. torch's current stream), so
 * that events recorded by the caller on that stream bracket the kernels. */
int pk_ctx_set_stream(pk_ctx* ctx, void* hip_stream);
int pk_sync(pk_ctx* ctx);
void pk_ctx_destroy(pk_ctx* ctx);

/* Per-kernel timing: when enabled every launch is bracketed by HIP events on
 * the context's stream.  pk_prof_read() synchronises and returns, for the
 * kernel class `name`, the number of launches and their summed duration (ms)
 * since the last pk_prof_reset().  Used by bench.py for roofline.achieved. */
int pk_prof_enable(pk_ctx* ctx, int on);
int pk_prof_reset(pk_ctx* ctx);
int pk_prof_read(pk_ctx* ctx, const char* name, int64_t* launches, double* total_ms);
/* Writes a '\n'-separated "name launches total_ms" listing into buf. */
int pk_prof_dump(pk_ctx* ctx, char* buf, int64_t buflen);

/* ------------------------------------------------------ Parallel WaveGAN */
/* Constructor arguments of PWGGenerator (parallel_wavegan.py:369-388) that
 * change device work.  Unsupported combinations -> PK_EUNSUPPORTED (the message names the limit).
 * The default 1/1/3/64/128/64/80 runs the tuned kernels (pwg.hip); every other shape inside the
 * envelope below runs the shape-generic kernels (pwg_gen.hip; also the default one under option
 * "generic_kernel"). */
typedef struct {
    int32_t in_channels;        /* 1 only */
    int32_t out_channels;       /* 1 only */
    int32_t kernel_size;        /* 3; odd, 1 ... 9 (padding (k-1)/2 * dilation) */
    int32_t layers;             /* 30, must be a multiple of stacks (:398); dilation 2^(layers/stacks - 1) <= 2^11 */
    int32_t stacks;             /* 3  */
    int32_t residual_channels;  /* 64; a multiple of 16, 16 ... 256 */
    int32_t gate_channels;      /* 128; 32 ... 512 with gate_channels / 2 a multiple of 16 */
    int32_t skip_channels;      /* 64; a multiple of 16, 16 ... 256 */
    int32_t aux_channels;       /* 80; 1 ... 512 */
    int32_t aux_context_window; /* 2 */
    int32_t n_upsample;         /* 4 */
    int32_t upsample_scales[8]; /* 4,4,4,4 (LJSpeech, hop 256) or 4,5,3,5 (baker / vctk, hop 300); any product 32..1024 */
    int32_t use_causal_conv;    /* 0 only (the reference's causal branch cannot run, :305) */
} pk_pwg_cfg;

int pk_pwg_create(pk_ctx* ctx, const pk_pwg_cfg* cfg, pk_pwg** out);
/* set_state_dict, one entry at a time.  `name` is the reference's state-dict
 * key ("conv_layers.3.conv.weight", "...weight_g", "...weight_v", ...);
 * float32 host data of the given shape. */
int pk_pwg_set_param(pk_pwg* h, const char* name, const float* data,
                     const int64_t* shape, int32_t ndim);
/* PWGInference's normalizer (ZScore, parakeet/modules/normalizer.py:18-33):
 * mel_in -> (mel_in - mu) / sigma.  NULL,NULL = identity. */
int pk_pwg_set_normalizer(pk_pwg* h, const float* mu, const float* sigma, int32_t n);
/* Arithmetic of the residual-block contractions (activations, weights, accumulators and every stored
 * tensor are fp32 in all modes).  Default PK_PWG_MATH_F16X3.
 *   PK_PWG_MATH_F32     exact fp32 products on v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain);
 *   PK_PWG_MATH_F16X3   each fp32 product as a_hi*b_hi + a_lo*b_hi + a_hi*b_lo with fp16 parts
 *                       (11 + 11 significant bits per operand, dropped term 2^-22) on
 *                       v_mfma_f32_32x32x16_f16, fp32 accumulation.  Measured on the 30-layer generator:
 *                       relative max error 7e-7 (rms 2.3e-7) vs the fp64 oracle -- the class of the exact
 *                       path (5e-7, rms 1.9e-7) and of a CPU fp32 run (6e-7).  5.3x less matrix-pipe time.
 *                       Operands are block scaled by powers of two before the split (csrc/pk_split.h): the
 *                       error does not depend on the magnitude of weights or activations (floor 2^-39 of the
 *                       block maximum, fp32 range);
 *   PK_PWG_MATH_BF16X3  the same with bf16 parts (fp32 range, 8 + 8 bits): error 3.7e-6. */
enum { PK_PWG_MATH_F32 = 0, PK_PWG_MATH_BF16X3 = 1, PK_PWG_MATH_F16X3 = 2 };
int pk_pwg_set_math(pk_pwg* h, int32_t mode);
/* Scheduling of the residual stack (no effect on results): the batch is processed in chunks of whole
 * utterances of at most `samples` samples, all layers over one chunk before the next, so that the chunk's
 * activations (768 B per sample) stay in the 256 MB Infinity Cache between layers (327 680 = two 7.4 s
 * utterances = 252 MB).  Default: one chunk (measured faster, see pwg.hip). */
int pk_pwg_set_chunk_samples(pk_pwg* h, int64_t samples);
/* Named integer options of a handle.  The library reads NO environment variable (the measurement / ablation switches of
 * earlier rounds exist only in the profile build, parakeet_amd/build.py build(profile=True)); what a caller may choose
 * is listed here.  Unknown key or value -> PK_EINVAL.
 *   "planes"       1 (default) = under PK_PWG_MATH_F16X3 the residual stream x is stored as pre-split fp16 planes at one
 *                  a-priori scale per utterance and layer (pwg.hip, k_pwg_tile_scales); 0 = x stored as fp32 with one
 *                  measured scale per 32-sample block (round 2's path: ~4 % slower, no magnitude bound involved).
 *   "scale_guard"  0 = off; 1 (default) = the FIRST inference after pk_pwg_finalize also measures max|x| per utterance and
 *                  layer on the planes path, and when the a-priori bound overshoots the measured maximum by more than
 *                  2^10 anywhere, the call is repeated on the "planes" = 0 path, which the handle then keeps; 2 = every call.
 *                  A guarded call synchronises the stream once and does two small blocking copies INSIDE pk_pwg_infer: the
 *                  first call after finalize stalls a pipelined caller and must not be stream-captured.
 *                  Under 1 every "scale_guard_every"-th later inference is SAMPLED as well (the layer kernel folds each layer's maxima
 *                  in from its epilogue on such calls: one extra small launch, not a pass over x per layer), its
 *                  verdict deferred: the maxima are copied to pinned host memory behind an event and judged at the start of
 *                  a later call -- no stall, no allocation (the pinned buffer, 0.5 MB for up to 4096 utterances, and the
 *                  event are created by pk_pwg_finalize; a call with more utterances is not sampled; a sample whose event
 *                  reports an error is dropped, not judged); a verdict above 2^10 moves the handle to the "planes" = 0
 *                  path from then on (the sampled call keeps its result: at 2^10 the planes still carry 26 bits of the
 *                  actual maximum).  A sampled call adds two device-to-host copies and an event record to the stream: like
 *                  a guarded call it must not be stream-captured (capture with "scale_guard" 0).
 *   "noise_fed_first"  1 (default) = on the "planes" path at hop 256 the first residual block is fed from the noise itself: first_conv is
 *                  Conv1D(1 -> 64, k = 1), so the block's dilated conv over x = w n + b is a 3-tap conv on n with weights folded (in fp64) by
 *                  pk_pwg_finalize -- no first_conv launch, no x planes for layer 0 (round 6); 0 = first_conv, then the ordinary first block.
 *                  Both are within the engine's error bars of the reference; they differ from each other in the last bits.
 *   "scale_guard_every"  the sampling period under "scale_guard" 1 (default 16; 0 = never re-sample).
 *   "fused_tail"   1 (default) = on the "planes" path at hop 256 (default math, layers >= 2, one chunk) the last residual block of a call that
 *                  is neither guarded nor sampled computes the waveform itself: last_conv_layers run on the skip sum in the block's registers,
 *                  the block's x_out and the finished skip sum are not stored and the separate last-layers launch is gone.  Same bits as
 *                  0 (= the ordinary last block, then the last-layers kernel).  pk_pwg_debug_read of taps 1, 2, 3 after a fused call first
 *                  runs the ordinary last block once on the handle's stream (its inputs are still in the workspace), so the taps are
 *                  those of 0 too.  No effect on the generic path.
 *   "generic_kernel"  1 = run the default shape on the shape-generic kernels as well (pwg_gen.hip; other shapes always
 *                  do); 0 (default) = the tuned kernels.  Takes effect at the next pk_pwg_finalize.  On the generic path
 *                  x is fp32 with a measured scale per 32-sample block under both split maths (the "planes" = 0 scheme):
 *                  "planes", "scale_guard", "scale_guard_every" and "noise_fed_first" are accepted and have no effect,
 *                  pk_pwg_scale_overshoot returns PK_ESTATE and debug tap 3 PK_EUNSUPPORTED.
 *                  pk_pwg_scale_overshoot reports what was measured. */
int pk_pwg_set_option(pk_pwg* h, const char* key, int64_t value);
/* log2(a-priori bound / measured max|x|) per layer input, l = 0 .. layers (n = layers + 1 floats), the maximum over the
 * utterances of the last guarded or sampled inference ("scale_guard"; a sample still in flight is waited for); *fell_back
 * (nullable) = 1 when the handle has left the planes path inside a guarded call, 2 when a deferred sample moved it there.
 * PK_ESTATE if no guarded inference has run. */
int pk_pwg_scale_overshoot(pk_pwg* h, float* log2_overshoot, int32_t n, int32_t* fell_back);
/* remove_weight_norm + packing into the kernels' layouts + upload. */
int pk_pwg_finalize(pk_pwg* h);
/* PWGGenerator.inference for a packed batch.
 *   mel    (sum(frames), aux_channels) float32, row-major, packed by utterance
 *          (with PK_PWG_C_HAS_CONTEXT: frames[b] + 2*ctx rows per utterance)
 *   frames (B) host int32, frames per utterance (>= 1)
 *   noise  (sum(frames)*hop) float32 packed; the x = randn(...) of :515-516, passed in so that
 *          results are reproducible; NULL = drawn internally (pk_randn stream of pk_pwg_set_seed)
 *   wav    (sum(frames)*hop) float32 packed output
 * flags: PK_HOST_IO if mel/noise/wav are host pointers. */
int pk_pwg_infer(pk_pwg* h, const float* mel, const int32_t* frames, int32_t B,
                 const float* noise, float* wav, int32_t flags);
/* Debug / test taps: copy internal activations of the LAST pk_pwg_infer call
 * for utterance b to host.  what: 0 = layer 0's conv1x1_aux(upsampled c) (gate_channels, S_b),
 * 1 = residual-stack output x (residual_channels, S_b), 2 = skip sum before the sqrt(1/layers)
 * scale (skip_channels, S_b), all channel-major. */
int pk_pwg_debug_read(pk_pwg* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_pwg_destroy(pk_pwg* h);

/* ------------------------------------------------------------ FastSpeech2 */
/* Constructor arguments of FastSpeech2 (fastspeech2.py:52-118) that change the
 * inference computation.  Dropout rates, init_type and the loss switches are
 * training-only and have no field.  Unsupported values -> PK_EUNSUPPORTED. */
typedef struct {
    int32_t idim, odim;
    int32_t adim, aheads;
    int32_t elayers, eunits, dlayers, dunits;
    int32_t positionwise_conv_kernel_size;
    int32_t positionwise_layer_type;            /* 0 "conv1d" (MultiLayeredConv1d), 1 "linear"
                                                 * (PositionwiseFeedForward), 2 "conv1d-linear" (Conv1dLinear);
                                                 * encoder.py:145-170 */
    int32_t duration_predictor_layers, duration_predictor_chans, duration_predictor_kernel_size;
    int32_t pitch_predictor_layers, pitch_predictor_chans, pitch_predictor_kernel_size;
    int32_t energy_predictor_layers, energy_predictor_chans, energy_predictor_kernel_size;
    int32_t pitch_embed_kernel_size, energy_embed_kernel_size;   /* 1 in every reference recipe */
    int32_t postnet_layers, postnet_chans, postnet_filts;
    int32_t use_batch_norm;
    int32_t use_scaled_pos_enc;
    int32_t encoder_normalize_before, decoder_normalize_before;  /* 0: post-norm blocks, no after_norm (encoder.py:142-143) */
    int32_t reduction_factor;                                    /* r mel frames per decoder row (feat_out: adim -> odim * r) */
    /* multi-speaker recipes (aishell3 / vctk: spk_embed_dim 256, "concat"): spk_embedding_table
     * [num_speakers, spk_embed_dim] (padding_idx 0) + spk_projection (fastspeech2.py:147-151,190-194). */
    int32_t num_speakers;                /* 0 with spk_embed_dim: only external embeddings (spembs) */
    int32_t spk_embed_dim;               /* 0 = single speaker */
    int32_t spk_embed_integration_type;  /* 0 = "add", 1 = "concat" */
    /* tone embedding (fastspeech2.py:153-157,197-202,404-408): tone_embedding_table [num_tones, tone_embed_dim]
     * (padding_idx 0) + tone_projection; only integration type "add" (0) -- with the 1-D tone ids that
     * FastSpeech2.inference forwards, the reference's "concat" branch (:606-610) cannot broadcast. */
    int32_t num_tones;
    int32_t tone_embed_dim;              /* 0 = no tone embedding */
    int32_t tone_embed_integration_type; /* 0 = "add" only */
    int32_t encoder_concat_after, decoder_concat_after;   /* concat_linear after the self-attention (encoder_layer.py:103-106) */
} pk_fs2_cfg;

int pk_fs2_create(pk_ctx* ctx, const pk_fs2_cfg* cfg, pk_fs2** out);
/* set_state_dict entry; names are the reference's keys ("encoder.encoders.0.self_attn.linear_q.weight", ...).
 * Linear weights are [in, out], Conv1D weights [Cout, Cin, k] (Paddle layouts). */
int pk_fs2_set_param(pk_fs2* h, const char* name, const float* data,
                     const int64_t* shape, int32_t ndim);
/* FastSpeech2Inference's normalizer: output mel -> mel * sigma + mu (ZScore.inverse,
 * fastspeech2.py:668-671).  NULL,NULL = return the normalised mel (FastSpeech2.inference). */
int pk_fs2_set_normalizer(pk_fs2* h, const float* mu, const float* sigma, int32_t n);
/* Arithmetic of the dense layers (Linear / Conv1D GEMMs) and of the two attention contractions: 0 = exact fp32
 * MFMA, 1 = block-scaled 3-term split-fp16 MFMA with fp32 accumulation (default; same construction and error
 * class as PK_PWG_MATH_F16X3; layers whose input channel count is not a multiple of 32 stay on the exact path).
 * LayerNorm, softmax, the duration arithmetic and every stored tensor are fp32 in both modes. */
int pk_fs2_set_math(pk_fs2* h, int32_t mode);
/* Named integer options (as pk_pwg_set_option; scheduling / tiling choices, results stay within the math mode's error class):
 *   "ffn_planes"             1 (default) = the feed-forward convs, q|k|v and attention-out projections of pre-norm FFT blocks
 *                            run on the planes kernels (csrc/ffn_planes.hip); 0 = on the tile GEMM
 *   "ffn_planes_min_blocks"  timelines shorter than this many 32-row blocks stay on the tile GEMM (default 0)
 *   "ffn_one_tile_max"       timelines with at most this many (32-row block, 32-column) tiles in a feed-forward conv run one tile
 *                            per wave (default 4096: the second conv up to sixteen utterances of 640 frames, the encoder's at thirty-two.  One
 *                            utterance 2.42 -> 2.0 ms, eight 3.1 -> 2.9, sixteen 3.73 -> 3.62, thirty-two 4.72 -> 4.64 on an MI355X;
 *                            8192 and more lose at thirty-two: four times the operand traffic per product); 0 = never
 *   "ffnp_variant"           0 (default) = tiling by shape; 88 / 84 / 48 / 44: first digit 8 / 4 = 256 / 128 output channels
 *                            per wave in the first conv, second digit = waves per workgroup of the second conv
 *   "attn_waves"             0 (default) = by shape; 4 / 8 query tiles per attention workgroup */
int pk_fs2_set_option(pk_fs2* h, const char* key, int64_t value);
int pk_fs2_finalize(pk_fs2* h);
/* Speaker conditioning of the NEXT pk_fs2_encode call (_forward :396-402, _integrate_with_spk_embed
 * :560-586): spk_id HOST int64 (B) looked up in spk_embedding_table, or spembs HOST float32
 * (B, spk_embed_dim) external embeddings (win over spk_id, as in the reference); both NULL (or never
 * called) = no integration, as when the reference gets neither.  B must equal the batch of that call;
 * the setting is consumed by it. */
int pk_fs2_set_speakers(pk_fs2* h, const int64_t* spk_id, const float* spembs, int32_t B);
/* Tone conditioning of the NEXT pk_fs2_encode call (:404-408, _integrate_with_tone_embed :588-604 with the
 * 1-D tone ids of FastSpeech2.inference: hs[t] += tone_projection(normalize(tone_embedding_table[tone[t]]))).
 * tone_id: HOST int64 packed by utterance like the token ids (n = sum of token counts); NULL clears. */
int pk_fs2_set_tones(pk_fs2* h, const int64_t* tone_id, int64_t n);
/* Given durations / pitch / energy of the NEXT pk_fs2_encode call: teacher forcing (_forward(..., ds, ps, es,
 * is_inference=False) :433-442) and prosody control.  HOST arrays packed by utterance like the token ids, n = sum of
 * token counts (another n -> PK_ESHAPE from that encode); each pointer may be NULL, all NULL clears; a negative duration
 * -> PK_EINVAL.  A given array stands in for the predictor's value of that quantity only, where it is consumed:
 * durations feed the prefix sums as they are -- no exp, no rounding, no alpha (length_regulator(hs, ds) :442; alpha
 * still scales PREDICTED durations) -- and count decoder rows: with reduction_factor r an utterance gets r * sum(d) mel
 * frames.  The predictors run all the same; with given durations the duration head writes DurationPredictor.forward
 * (log domain, masked to 0, unrounded; duration_predictor.py:85-103), the d_outs _forward returns in that mode.
 * The setting is consumed by the encode, whether it succeeds or not. */
int pk_fs2_set_targets(pk_fs2* h, const int64_t* durations, const float* pitch, const float* energy, int64_t n);
/* Phase 1 of inference (_forward :390-432): encoder, pitch/energy/duration predictors, prefix
 * sums.  ids: HOST int64, packed by utterance (sum(tok_lens)); tok_lens: HOST (B).
 * alpha = LengthRegulator speed control.  out_frames (HOST, B) receives the number of mel
 * frames of each utterance -- the output length is data dependent, so this call synchronises. */
int pk_fs2_encode(pk_fs2* h, const int64_t* ids, const int32_t* tok_lens, int32_t B, float alpha,
                  int32_t* out_frames);
/* Phase 2 (:432-466): length regulator, decoder, feat_out, postnet, (de)normalisation.
 * mel_out: (sum(out_frames), odim) float32 packed by utterance; device pointer, or host with
 * PK_HOST_IO. */
int pk_fs2_decode(pk_fs2* h, float* mel_out, int32_t flags);
/* The predictor outputs of the last pk_fs2_encode for the whole batch (d_outs, p_outs, e_outs of _forward :410-433):
 * HOST arrays of n = sum(tok_lens) floats packed by utterance, each may be NULL.  d_outs: the integer durations of the
 * inference branch (alpha applied), or the log-domain output when durations were given.  Needs no decode. */
int pk_fs2_read_predictions(pk_fs2* h, float* d_outs, float* p_outs, float* e_outs, int64_t n);
/* before_outs of the last pk_fs2_decode (:457, never de-normalised), packed like its mel: (sum(out_frames), odim),
 * device pointer, or host with PK_HOST_IO.  A model without postnet has no separate tensor (after_outs IS before_outs,
 * :460-461) -> PK_ESTATE. */
int pk_fs2_read_before(pk_fs2* h, float* before_out, int32_t flags);
/* Test taps of the last encode/decode for utterance b, copied to host:
 * 0 hs (T,adim) | 1 pitch (T) | 2 energy (T) | 3 durations (T) | 4 length-regulated hs (L,adim; needs
 * pk_fs2_set_debug(1)) | 5 decoder output (L,adim) | 6 before_outs (L,odim). */
int pk_fs2_set_debug(pk_fs2* h, int32_t on);
int pk_fs2_debug_read(pk_fs2* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_fs2_destroy(pk_fs2* h);

/* --------------------------------------------------------------- WaveFlow */
/* Constructor arguments of ConditionalWaveFlow (waveflow.py:741-757). */
typedef struct {
    int32_t n_upsample;
    int32_t upsample_factors[4];   /* 16, 16 */
    int32_t n_flows;               /* 8, even (:586-589) */
    int32_t n_layers;              /* 8 = len(dilations_dict[n_group]) (:328-331) */
    int32_t n_group;               /* 8, 16, 32, 64 or 128: the keys of Flow.dilations_dict (:420-426), which gives residual layer l
                                    * its height dilation -- 1 for every layer up to 16; 1 2 4 1 2 4 1 2 at 32; 1 2 4 8 16 1 2 4 at
                                    * 64; 1 2 4 8 16 32 64 1 at 128.  Another even value: PK_EUNSUPPORTED (a KeyError there); odd:
                                    * PK_EINVAL (:586-589) */
    int32_t channels;              /* 64 (paper small model) / 128 (repo default) */
    int32_t n_mels;                /* 80; a multiple of 16 up to 256 (the upsampling kernel's block), else PK_EUNSUPPORTED */
    int32_t kernel_h, kernel_w;    /* 3, 3 */
} pk_wf_cfg;

int pk_wf_create(pk_ctx* ctx, const pk_wf_cfg* cfg, pk_wf** out);
/* state-dict keys of ConditionalWaveFlow: encoder.{i}.*, decoder.{f}.input_proj.*,
 * decoder.{f}.resnet.{l}.{conv,condition_proj,out_proj}.*, decoder.{f}.output_proj.*;
 * weight_g / weight_v pairs are folded (recursively_remove_weight_norm). */
int pk_wf_set_param(pk_wf* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* 0 = exact fp32 MFMA, 1 = 3-term split-fp16 MFMA products with fp32 accumulation (default: fp32-equivalent error, as
 * pk_fs2_set_math), 2 = fp16 operands rounded to nearest, ONE MFMA per product, fp32 accumulation -- the precision the
 * reference itself synthesises at (examples/waveflow/synthesize.py:40 runs under paddle.amp.auto_cast), about 1e-4 of the
 * waveform's peak away from the fp64 oracle; 64- and 128-channel models only (PK_EUNSUPPORTED otherwise). */
int pk_wf_set_math(pk_wf* h, int32_t mode);
/* Named integer options (as pk_pwg_set_option; scheduling only, results do not change):
 *   "layer_waves"  0 (default) = the fused layer kernel of the 64-channel model runs in 12-wave workgroups (three waves per SIMD)
 *                  where that saves a round over 8-wave ones (BASELINE config 5's 8 x 640 frames: 11 tiles per workgroup), in both
 *                  maths; 6 / 8 / 12 = forced (6: two 6-wave workgroups per CU).  Same waveform bit for bit whatever the value.
 *                  (Round 5 refused three waves per SIMD in the default math: sporadic wrong tiles.  Round 6 found the cause -- a
 *                  packed fp32 FMA with op_sel, DESIGN.md 4.3 "the op_sel rule" -- and every configuration is back.)
 *   "persistent"   0 only.  (1 = the layers of a row in ONE cooperative launch with a barrier across the grid between two layers:
 *                  measured slower than eight launches in round 4; PK_EUNSUPPORTED in the product, a measurement configuration of
 *                  the profile build, and there for n_group 8 / 16 only: the launch has one tap table for all its layers)
 *   "fuse_step"    1 (default) = a row's affine step and the next row's input projection happen in the launch of its last
 *                  layer; 0 = in a kernel of their own
 *   "keep_cond"    0 (default); 1 = pk_wf_infer on the fused layer kernel, which turns the upsampled condition into fp16 planes in
 *                  place, first keeps a copy of it for pk_wf_debug_read (a test tap: one more buffer and a copy per call) */
int pk_wf_set_option(pk_wf* h, const char* key, int64_t value);
int pk_wf_finalize(pk_wf* h);
/* For t_mel frames: length of the trimmed upsampled condition (= length of the z the reference
 * draws, waveflow.py:799-801) and of the returned waveform (pruned to a multiple of n_group, :695). */
int pk_wf_cond_length(pk_wf* h, int32_t t_mel, int32_t* cond_len, int32_t* wav_len);
/* ConditionalWaveFlow.infer (:785-805) for a packed batch.
 *   mel    (sum(frames), n_mels) float32 packed by utterance, time-major (the reference's
 *          (B, C_mel, T_mel) transposed)
 *   frames (B) host int32, >= 2
 *   z      packed latent, cond_len(frames[b]) floats per utterance (the randn of :801);
 *          NULL = drawn internally (pk_randn stream of pk_wf_set_seed)
 *   wav    packed output, wav_len(frames[b]) floats per utterance
 * Every n_group of pk_wf_cfg: a layer with height dilation dh looks back at the rows i - dh and i - 2 dh of its own input, kept in
 * a ring of min(2 dh + 1, n_group) rows per layer -- the workspace is sum of the rings (25 rows of positions x channels floats
 * up to n_group 16, 264 at n_group 128) and the launch count n_flows x (n_group - 1) x n_layers whatever the dilations. */
int pk_wf_infer(pk_wf* h, const float* mel, const int32_t* frames, int32_t B, const float* z,
                float* wav, int32_t flags);
/* ConditionalWaveFlow.forward (:759-782): density estimation, audio -> (z, log-determinant), for a packed ragged batch.  Not
 * autoregressive: a layer of a flow runs on all n_group - 1 rows in one launch (n_flows x n_layers dependent layer launches, for
 * every n_group: the rows lie behind 2 x the largest height dilation rows of zeros, the conv's causal padding).
 *   mel, frames  as pk_wf_infer (frames >= 1); the condition is the UNTRIMMED upsampled mel (:780), frames[b] * prod(factors) long
 *   audio        packed, audio_len[b] floats per utterance; n_group <= audio_len[b] <= frames[b] * prod(factors) (_trim :617-625),
 *                else PK_EINVAL
 *   z            packed output, audio_len[b] / n_group * n_group floats per utterance (pk_wf_forward_length)
 *   logdet       (B) DOUBLE: sum of logs over the flows, rows and positions of utterance b (the reference returns their sum over the
 *                batch, :671).  Fixed summation order: the same bits for an utterance in any batch, as z.
 * Pointers are device memory, or host with PK_HOST_IO (frames / audio_len are always host).  PK_ESTATE before pk_wf_finalize. */
int pk_wf_forward_length(pk_wf* h, int32_t t_mel, int32_t n_audio, int32_t* z_len);
int pk_wf_forward(pk_wf* h, const float* mel, const int32_t* frames, const float* audio, const int32_t* audio_len, int32_t B,
                  float* z, double* logdet, int32_t flags);
/* Test tap of the last pk_wf_infer / pk_wf_forward for utterance b, copied to host: what = 0 is the upsampled condition as the
 * flows read it, (n_mels, wav_len) in natural time order -- after pk_wf_infer the trimmed upsampling cut to wav_len, after
 * pk_wf_forward the untrimmed one cut to the z length.  Un-folds both layouts of the condition buffer ([pos][mp] and the fused
 * path's blocks of 32 positions).  PK_ESTATE before a call has run, and after a pk_wf_infer on the fused layer kernel without
 * option "keep_cond". */
int pk_wf_debug_read(pk_wf* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_wf_destroy(pk_wf* h);

/* ------------------------------------------------------------ SpeedySpeech */
/* SpeedySpeech(vocab_size, encoder_hidden_size, encoder_kernel_size, encoder_dilations,
 * duration_predictor_hidden_size, decoder_hidden_size, decoder_output_size, decoder_kernel_size,
 * decoder_dilations, tone_size) -- parakeet/models/speedyspeech/speedyspeech.py:142-166. */
typedef struct {
    int32_t vocab_size;
    int32_t tone_size;                    /* 0 = no tone embedding (tone_size=None) */
    int32_t encoder_hidden_size, encoder_kernel_size, n_encoder_dilations;
    int32_t encoder_dilations[32];
    int32_t duration_predictor_hidden_size;
    int32_t decoder_hidden_size, decoder_output_size, decoder_kernel_size, n_decoder_dilations;
    int32_t decoder_dilations[32];
    /* Every convolution of the model is nn.Conv1D(..., dilation=d, padding="same").  Paddle's conv kernels
     * (UpdatePaddingAndDilation, paddle/fluid/operators/conv_op.h, release 2.1) compute the "SAME" pads from
     * the undilated kernel -- before = (k-1)/2, after = (k-1) - before -- and RESET THE DILATION TO 1, so the
     * reference as it runs on Paddle does not dilate [paddle-semantics, unverified: Paddle is not installable
     * in the build image].  1 = that behaviour (what released checkpoints were trained with), 0 = the
     * convolution as written: dilation d, pads d*(k-1) split the same way. */
    int32_t same_padding_resets_dilation;
} pk_ss_cfg;
typedef struct pk_ss pk_ss;

int pk_ss_create(pk_ctx* ctx, const pk_ss_cfg* cfg, pk_ss** out);
/* set_state_dict entry ("encoder.res_blocks.3.blocks.1.0.weight", "...2._variance", ...). */
int pk_ss_set_param(pk_ss* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* SpeedySpeechInference's normalizer (:221-231): mel -> mel * sigma + mu.  NULL,NULL = SpeedySpeech.inference. */
int pk_ss_set_normalizer(pk_ss* h, const float* mu, const float* sigma, int32_t n);
/* 0 = exact fp32 MFMA, 1 = 3-term split-fp16 MFMA GEMMs (default, as pk_fs2_set_math). */
int pk_ss_set_math(pk_ss* h, int32_t mode);
int pk_ss_finalize(pk_ss* h);
/* Phase 1 of SpeedySpeech.inference (:178-196) for a packed batch: encoder, duration predictor,
 * durations = round(exp(.)).  text / tones: HOST int64, packed by utterance (tones may be NULL, :183);
 * tok_lens: HOST (B).  out_frames (B) host: decoder lengths (the sync the reference has at :194-196). */
int pk_ss_encode(pk_ss* h, const int64_t* text, const int64_t* tones, const int32_t* tok_lens, int32_t B,
                 int32_t* out_frames);
/* Phase 2 (:197-218): expand, + sinusoid_position_encoding, decoder -> packed (sum(frames), output_size). */
int pk_ss_decode(pk_ss* h, float* mel_out, int32_t flags);
/* SpeedySpeech.forward (:166-184): pk_ss_encode with the durations given by the caller.  The duration predictor still
 * runs (forward returns pred_durations: pk_ss_pred_durations); the given durations stand where the head's would, and
 * pk_ss_decode follows as after pk_ss_encode.  durations: HOST int64, packed like text, every value >= 0 (PK_EINVAL
 * otherwise); a duration of 0 owns no frame (expansion.py:33).  frame_lens: HOST (B) or NULL.  NULL: utterance b decodes
 * sum(d_b) frames, each utterance as if it were alone (forward at B = 1).  Otherwise it decodes frame_lens[b] >= sum(d_b)
 * frames (smaller: PK_EINVAL); the frames past sum(d_b) are zero rows plus the positional encoding and take part in every
 * convolution.  That is one row of the reference's batched forward, which has no masks: pass the padded ids (id 0 embeds
 * to zero), tok_lens = T_max and frame_lens = max_b sum(d_b) to reproduce it.  out_frames (B) host: the decoder lengths;
 * they are known on the host, so the call does not wait for the device. */
int pk_ss_encode_given(pk_ss* h, const int64_t* text, const int64_t* tones, const int32_t* tok_lens,
                       const int64_t* durations, const int32_t* frame_lens, int32_t B, int32_t* out_frames);
/* Packed (sum tok_lens) log-durations the duration predictor gave in the last encode; PK_HOST_IO honoured. */
int pk_ss_pred_durations(pk_ss* h, float* out, int32_t flags);
/* The evaluator's text_mask (speedyspeech_updater.py:122-123): the next pk_ss_duration_loss sums over the first
 * n_valid[b] <= tok_lens[b] tokens of utterance b.  HOST (B); NULL = all tokens, which every encode restores. */
int pk_ss_set_valid_tokens(pk_ss* h, const int32_t* n_valid, int32_t B);
/* sums_out (B) double: sum over the utterance's tokens of huber_loss(pred, log(max(d, 1)), delta = 1)
 * (paddle.fluid.layers.huber_loss: r = label - input; 0.5 r^2 for |r| <= 1, |r| - 0.5 beyond) of the last
 * pk_ss_encode_given (speedyspeech_updater.py:129-136).  After a plain pk_ss_encode: PK_ESTATE.  The tokens are those
 * pk_ss_set_valid_tokens named SINCE the last encode; every encode resets them to all tokens, so set them after
 * pk_ss_encode_given and before this call. */
int pk_ss_duration_loss(pk_ss* h, double* sums_out, int32_t flags);
/* Test taps of the last encode: 0 = encodings (T_b, H), 1 = log-durations (T_b), 2 = durations (T_b). */
int pk_ss_debug_read(pk_ss* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_ss_destroy(pk_ss* h);

/* ----------------------------------------------------------- dropout stream */
/* Tacotron2-style decoder prenets keep dropout ON at inference -- TransformerTTS through
 * modules/tacotron2/decoder.py:78-81 (F.dropout(x): p = 0.5, training = True whatever model.eval() says),
 * Tacotron2 through models/tacotron2.py:76-79 (training=True) -- so the reference's outputs depend on Paddle's
 * generator.  The engine draws the masks from a counter-based stream instead, a pure function of (seed, element
 * index): Philox4x32-10 with key = seed and counter = (lo(e >> 2), hi(e >> 2), 0, 0x44524F50); element e uses
 * word e & 3 of that block; keep <=> word >= floor(p * 2^32); kept values are multiplied by 1 / (1 - p)
 * (upscale_in_train, paddle.nn.functional.dropout's default mode).  oracle/philox_ref.py restates it; the golden
 * vectors of tests/golden/ come from the reference source run with this stream injected.
 * The element index of a model is stated with its entry point. */

/* ----------------------------------------------------------- TransformerTTS */
/* TransformerTTS(idim, odim, **model_cfg) -- parakeet/models/transformer_tts/transformer_tts.py:172-358.
 * Built: the embedding or conv-prenet encoder input layer, pre-norm blocks, the decoder prenet, the stop token,
 * the postnet, speaker embeddings ("add" / "concat"), both positional encodings, the "linear" decoder input layer
 * (dprenet_layers == 0), reduction_factor >= 1, global style tokens (use_gst: modules/style_encoder.py), post-norm and
 * concat_after blocks in the encoder and the decoder (encoder_layer.py:64-115, decoder_layer.py:104-151). */
typedef struct {
    int32_t idim, odim;
    int32_t embed_dim, eprenet_conv_layers, eprenet_conv_chans, eprenet_conv_filts;   /* layers 0: nn.Embedding(idim, adim) (:272-277) */
    int32_t dprenet_layers, dprenet_units;
    int32_t adim, aheads;
    int32_t elayers, eunits, dlayers, dunits;
    int32_t postnet_layers, postnet_chans, postnet_filts;
    int32_t positionwise_layer_type;       /* encoder only, 0 conv1d, 1 linear, 2 conv1d-linear (encoder.py:145-170) */
    int32_t positionwise_conv_kernel_size;
    int32_t use_scaled_pos_enc, use_batch_norm;
    int32_t encoder_normalize_before, decoder_normalize_before;
    int32_t encoder_concat_after, decoder_concat_after;
    int32_t reduction_factor;
    int32_t spk_embed_dim;                 /* 0 = None */
    int32_t use_gst;
    int32_t spk_embed_integration_type;    /* 0 = "add", 1 = "concat" (:313-317) */
    /* StyleEncoder(idim=odim, gst_token_dim=adim, ...) (:299-310), read when use_gst != 0 */
    int32_t gst_tokens, gst_heads;
    int32_t gst_conv_layers, gst_conv_kernel_size, gst_conv_stride;
    int32_t gst_gru_layers, gst_gru_units;
    int32_t gst_conv_chans[8];             /* gst_conv_chans_list, gst_conv_layers entries used */
} pk_tts_cfg;
typedef struct pk_tts pk_tts;

int pk_tts_create(pk_ctx* ctx, const pk_tts_cfg* cfg, pk_tts** out);
/* set_state_dict entry ("decoder.decoders.2.src_attn.linear_q.weight", "decoder.embed.0.0.prenet.1.0.bias", ...). */
int pk_tts_set_param(pk_tts* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* TransformerTTSInference's normalizer (:757-767): mel -> mel * sigma + mu, applied by pk_tts_read under
 * PK_APPLY_NORMALIZER.  NULL,NULL removes it. */
int pk_tts_set_normalizer(pk_tts* h, const float* mu, const float* sigma, int32_t n);
/* 0 = exact fp32 MFMA, 1 = 3-term split-fp16 MFMA GEMMs (default, as pk_fs2_set_math). */
int pk_tts_set_math(pk_tts* h, int32_t mode);
/* Named integer options: those of pk_fs2_set_option (the encoder's FFT stack), and
 *   "kv_prefix"  0 (default); 1 = decoder layer 0 projects k | v only for the prefix rows and q for the new rows with a
 *                row GEMM (measured neutral on an MI355X, kept as an option)
 *   "overlap_prefix"  1 (default) = the next decoding step's prefix work (prenet with its fresh dropout, input layer, layer 0's
 *                q | k | v of the row blocks that exist already) runs on a side stream under the current step's layer chain;
 *                0 = everything in order on one stream.  Same spectrogram bit for bit
 *   "fuse_prenet"  1 (default) = the decoder prenet (two layers) and the input layer of a step's new rows run as one launch;
 *                0 = three row GEMMs.  Same result up to summation order
 *   "fuse_src_q"  1 (default) = with 64-wide heads, at most 256 memory rows and adim <= 512 the encoder-decoder attention of a
 *                decoding step projects its own query (norm2 + linear_q inside the attention kernel: one launch less per layer);
 *                0 = a row GEMM of its own.  Same result up to summation order
 *   "overlap_cu_mask"  0 (default) = that side stream is an ordinary stream at the least urgent priority, the decoding loop's own
 *                stream at the most urgent; 1 = the side stream is confined to every other CU; 2 = and the loop's stream to the
 *                others.  Measured within 3 % of one another on an MI355X.  Read when the streams are created */
int pk_tts_set_option(pk_tts* h, const char* key, int64_t value);
/* Decoder-prenet dropout: 1 (default) = the dropout stream above with p = 0.5, element index
 * ((s*(s-1)/2 + pos) * dprenet_layers + layer) * dprenet_units + unit for decoding step s = 1, 2, ... and prefix
 * position pos < s (the reference re-applies the prenet to the whole prefix at every step, decoder.py:210);
 * 0 = no dropout (deterministic variant; not what the reference computes). */
int pk_tts_set_dropout(pk_tts* h, int32_t on);
int pk_tts_finalize(pk_tts* h);
/* Speaker embeddings of the NEXT pk_tts_infer call (_integrate_with_spk_embed :725-755, applied to the encoder output
 * :591-593): spembs HOST float32 (B, spk_embed_dim), one row per utterance.  Consumed by that call; NULL clears it.
 * A model with spk_embed_dim > 0 refuses to infer without them (the reference fails on spemb = None). */
int pk_tts_set_speakers(pk_tts* h, const float* spembs, int32_t B);
/* Reference spectrograms of the NEXT pk_tts_infer call for a use_gst model (`speech` of inference(), :586-588): speech
 * HOST float32 packed (sum(lens), odim), lens HOST (B) frames per utterance.  Consumed by that call; NULL clears it. */
int pk_tts_set_style_reference(pk_tts* h, const float* speech, const int32_t* lens, int32_t B);
/* TransformerTTS.inference (:511-647) for a packed batch, up to (not including) the postnet: <eos> = idim - 1 is
 * appended to every utterance (:563-565), the encoder runs once, then the decoder is stepped until every utterance
 * has stopped: utterance b ends at the first step s >= int(T_b * minlenratio) with sigmoid(prob_out) >= threshold
 * or s >= int(T_b * maxlenratio), T_b counting <eos> (:597-598, :638-642).
 *   ids      HOST int64, packed by utterance, WITHOUT <eos>;  tok_lens HOST (B)
 *   seeds    HOST (B) dropout-stream seed per utterance, or NULL = seed 0 for every utterance
 *   out_frames (B) host: L_b = decoder steps * reduction_factor (the per-step sync the reference has at :638)
 * flags: PK_TTS_KEEP_ATT keeps the encoder-decoder attention weights for pk_tts_read. */
int pk_tts_infer(pk_tts* h, const int64_t* ids, const int32_t* tok_lens, int32_t B, double threshold,
                 double minlenratio, double maxlenratio, const uint64_t* seeds, int32_t flags, int32_t* out_frames);
/* TransformerTTS.inference(..., use_teacher_forcing=True) (:567-579 -> _forward :462-500) for a packed batch, up to (not
 * including) the postnet.  <eos> is appended as in pk_tts_infer; the style embedding of a use_gst model comes from the
 * teacher spectrogram itself (self.gst(ys), :475-477); the decoder inputs are ys[:, r - 1::r] with a zero frame in front and
 * the last row dropped (:484-492), and the whole decoder runs as one pass under the causal target mask (:692-723).  Prenet
 * dropout stays on: the prenet sees the L_b / r rows of an utterance in one call, the dropout-stream elements of the AR
 * decode's call at step s = L_b / r.
 *   ids, tok_lens, seeds  as pk_tts_infer
 *   speech       float32 packed (sum(L_b), odim) teacher spectrograms in the model's normalised space: device memory, or
 *                host memory under PK_HOST_IO (a use_gst model copies device speech to the host for its style encoder)
 *   speech_lens  HOST (B) frames L_b >= reduction_factor
 *   out_frames   (B) host: (L_b / reduction_factor) * reduction_factor (known up front: no device sync)
 * Consumes the pending pk_tts_set_speakers rows (required by a model with spk_embed_dim) and drops a pending
 * pk_tts_set_style_reference.  pk_tts_read (probabilities: the stop head on the teacher-forced rows, an engine extra; the
 * reference returns None) and pk_tts_debug_read then serve its result.  Refused: more tokens than the AR decode's
 * attention kernels hold (PK_EUNSUPPORTED), L_b < reduction_factor (PK_EINVAL).
 * flags: PK_TTS_KEEP_ATT keeps the encoder-decoder attention weights, PK_HOST_IO for `speech`. */
int pk_tts_teacher(pk_tts* h, const int64_t* ids, const int32_t* tok_lens, int32_t B, const float* speech,
                   const int32_t* speech_lens, const uint64_t* seeds, int32_t flags, int32_t* out_frames);
/* Postnet + outputs of the last pk_tts_infer or pk_tts_teacher (:644-651).
 *   mel_out   packed (sum(L_b), odim): outs + postnet(outs), de-normalised under PK_APPLY_NORMALIZER
 *   probs_out packed (sum(L_b)) stop probabilities, or NULL
 *   att_out   per utterance (dlayers, aheads, L_b / reduction_factor, T_b) encoder-decoder attention weights (one row
 *             per decoder step, :623-636), utterances one after another, or NULL; needs PK_TTS_KEEP_ATT at infer
 * flags: PK_HOST_IO if the three are host pointers. */
int pk_tts_read(pk_tts* h, float* mel_out, float* probs_out, float* att_out, int32_t flags);
/* What the criterion needs of the last pk_tts_teacher beside pk_tts_read's outputs (TransformerTTSLoss, :801): before_out
 * packed (sum frames, odim), the outputs before the postnet (:498), never de-normalised; logits_out packed (sum frames), the
 * stop head BEFORE the sigmoid (:500) -- pk_tts_read's probabilities are sigmoid(these), and saturate where these do not.
 * Either may be NULL.  Device pointers, or host pointers under PK_HOST_IO (then synchronous).  PK_ESTATE unless the handle's
 * last completed call was pk_tts_teacher (the autoregressive decode keeps no logits). */
int pk_tts_read_teacher(pk_tts* h, float* before_out, float* logits_out, int32_t flags);
/* Test taps of the last infer: 0 = encoder output hs (T_b, adim), 1 = outs before the postnet (L_b, odim),
 * 2 = last decoder layer's output rows (L_b / reduction_factor, adim). */
int pk_tts_debug_read(pk_tts* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_tts_destroy(pk_tts* h);

/* ---------------------------------------------------------------- Tacotron2 */
/* Tacotron2(vocab_size, n_tones, d_mels, d_encoder, ...) -- parakeet/models/tacotron2.py:626-689.
 * Refused with PK_EUNSUPPORTED: reduction_factor != 1 (Tacotron2.infer itself cannot run it: the postnet receives the
 * (B, T, d_mels * r) decoder output, :822-826). */
typedef struct {
    int32_t vocab_size;
    int32_t n_tones;                 /* 0 = None */
    int32_t d_mels, reduction_factor;
    int32_t d_encoder, encoder_conv_layers, encoder_kernel_size;
    int32_t d_prenet, d_attention_rnn, d_decoder_rnn;
    int32_t d_attention, attention_filters, attention_kernel_size;
    int32_t d_postnet, postnet_kernel_size, postnet_conv_layers;
    int32_t d_global_condition;      /* 0 = None; else a multiple of 16: the decoder's memory is d_encoder + this wide (:668-669) */
    int32_t use_stop_token;
    float p_prenet_dropout;          /* DecoderPreNet applies it with training=True (:76-79) */
} pk_taco_cfg;
typedef struct pk_taco pk_taco;

int pk_taco_create(pk_ctx* ctx, const pk_taco_cfg* cfg, pk_taco** out);
/* set_state_dict entry.  paddle.nn.LSTM registers each cell parameter twice ("encoder.lstm.0.cell_fw.weight_ih" and
 * "encoder.lstm.weight_ih_l0"); either name is accepted, the cuDNN-style one wins when both are given. */
int pk_taco_set_param(pk_taco* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* 0 = exact fp32 MFMA, 1 = 3-term split-fp16 MFMA GEMMs (default, as pk_fs2_set_math). */
int pk_taco_set_math(pk_taco* h, int32_t mode);
/* Decoder-prenet dropout: 1 (default) = the dropout stream with p = p_prenet_dropout, element index
 * (step * 2 + layer) * d_prenet + unit for decoding step 0, 1, ...; 0 = no dropout (not what the reference computes). */
int pk_taco_set_dropout(pk_taco* h, int32_t on);
int pk_taco_finalize(pk_taco* h);
/* Global condition of the NEXT pk_taco_infer / pk_taco_teacher call (:816-821): g HOST float32 (B, d_global_condition), one row per
 * utterance, concatenated to every encoder output row of that utterance.  Consumed by that call; NULL clears it.
 * A model with d_global_condition > 0 refuses to infer without it (the reference fails on the shapes). */
int pk_taco_set_global_condition(pk_taco* h, const float* g, int32_t B);
/* Tacotron2.infer (:781-840) for a packed batch, up to (not including) the postnet: embedding (+ tones), encoder
 * (conv stack, bidirectional LSTM), then the attention decoder is stepped in lockstep until every utterance has
 * ended: sigmoid(stop_logit) > 0.5 with a stop token (:515-518), else the "content exhausted" rule on the argmax of
 * the alignment (:520-525), or max_decoder_steps (:526-528).
 *   ids / tones  HOST int64, packed by utterance (tones NULL unless n_tones > 0);  tok_lens HOST (B)
 *   seeds        HOST (B) dropout-stream seed per utterance, or NULL = 0
 *   out_frames   (B) host: decoder steps L_b */
int pk_taco_infer(pk_taco* h, const int64_t* ids, const int64_t* tones, const int32_t* tok_lens, int32_t B,
                  int32_t max_decoder_steps, const uint64_t* seeds, int32_t flags, int32_t* out_frames);
/* Tacotron2.forward (:691-778) with eval semantics for a packed batch, up to the postnet: the decoder is teacher-forced
 * (Tacotron2Decoder.forward :419-472), the query of step s is [0, mels[0], ..., mels[L_b - 2]][s] and not the decoder's
 * own previous output; exactly L_b steps, no stop rule (with a stop token the logit of every step is recorded).  The
 * prenet of all sum(L_b) query rows runs in one launch before the loop, every row bit-identical to what pk_taco_infer's
 * per-step prenet gives for the same query, step and seed; the loop of max(L_b) steps is enqueued without a host poll.
 *   ids / tones / tok_lens / seeds  as pk_taco_infer
 *   mels         packed (sum(L_b), d_mels) float32 in the model's mel domain; device, or host under PK_HOST_IO
 *   frame_lens   HOST (B) teacher frames L_b >= 1
 *   out_frames   (B) host: L_b
 * Consumes the pending pk_taco_set_global_condition rows like pk_taco_infer.  pk_taco_read and pk_taco_debug_read then
 * serve its result. */
int pk_taco_teacher(pk_taco* h, const int64_t* ids, const int64_t* tones, const int32_t* tok_lens, int32_t B,
                    const float* mels, const int32_t* frame_lens, const uint64_t* seeds, int32_t flags, int32_t* out_frames);
/* Outputs of the last pk_taco_infer or pk_taco_teacher (:825-838), each packed by utterance, any of them may be NULL:
 *   mel_output (sum(L_b), d_mels); mel_outputs_postnet = mel_output + postnet(mel_output), same shape;
 *   alignments: per utterance (L_b, T_b); stop_logits (sum(L_b)), only with a stop token.
 * flags: PK_HOST_IO if they are host pointers. */
int pk_taco_read(pk_taco* h, float* mel_output, float* mel_outputs_postnet, float* alignments, float* stop_logits,
                 int32_t flags);
/* Test tap of the last infer: 0 = encoder outputs (T_b, d_encoder). */
int pk_taco_debug_read(pk_taco* h, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pk_taco_destroy(pk_taco* h);

/* ------------------------------------------------------- GE2E speaker encoder */
/* LSTMSpeakerEncoder(n_mels, num_layers, hidden_size, output_size) -- parakeet/models/lstm_speaker_encoder.py:24-53
 * (released config examples/ge2e/config.py: 40, 3, 256, 256).  Forward only: embed_sequences / embed_utterance and the GE2E
 * similarity matrix and loss (no gradients).
 * Refused with PK_EUNSUPPORTED: hidden_size not a multiple of 32 or above 512, output_size not a multiple of 32 or above
 * 4096, n_mels above 4096. */
typedef struct {
    int32_t n_mels, num_layers, hidden_size, output_size;
} pk_spk_cfg;
typedef struct pk_spk pk_spk;

int pk_spk_create(pk_ctx* ctx, const pk_spk_cfg* cfg, pk_spk** out);
/* set_state_dict entry: lstm.weight_ih_l{k} / weight_hh_l{k} / bias_ih_l{k} / bias_hh_l{k} (or their aliases
 * lstm.{k}.cell.weight_ih ...; the first form wins when both are given), linear.weight [in, out], linear.bias.
 * similarity_weight / similarity_bias (:29-32): shape [1] (else PK_ESHAPE), 10 and -5 unless set; read by pk_spk_ge2e, and
 * setting them does not ask for another pk_spk_finalize.  Other names are stored and ignored. */
int pk_spk_set_param(pk_spk* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* 0 = exact fp32 MFMA, 1 = 3-term split-fp16 MFMA (default, as pk_taco_set_math). */
int pk_spk_set_math(pk_spk* h, int32_t mode);
int pk_spk_finalize(pk_spk* h);
/* embed_sequences (:40-48) of P partials of T frames, all pointers but cu_partials on the DEVICE:
 *   partials  (P, T, n_mels) float32
 *   h0, c0    (num_layers, P, hidden_size) initial states, or both NULL (zeros)
 *   cu_partials HOST (U + 1): utterance u = partials cu[u] .. cu[u + 1] - 1 -> out (U, output_size) = embed_utterance of
 *             each (:50-53: mean of the normalised partial embeddings, normalised again); NULL: U == P and out (P,
 *             output_size) = the normalised partial embeddings.
 * A partial's embedding does not depend on the other partials of the call. */
int pk_spk_embed(pk_spk* h, const float* partials, int32_t P, int32_t T, const float* h0, const float* c0,
                 const int32_t* cu_partials, int32_t U, float* out);
/* similarity_matrix (:55-104) and the softmax loss (:122-134) of embeds (N, M, C) float32 on the DEVICE: N speakers of M
 * utterances, C dimensions, not assumed unit-norm.  Needs no pk_spk_finalize.  Outputs, each a DEVICE pointer or NULL
 * (nothing is stored for a NULL one):
 *   sim     (N*M, N)  p = (p1 with the own-speaker column replaced by p2) * similarity_weight + similarity_bias
 *   p1      (N*M*N)   e . normalised inclusive centroid of every speaker
 *   p2      (N*M)     e . normalised exclusive centroid (sum_m e - e) / (M - 1) of its own speaker
 *   row_nll (N*M)     float64 logsumexp(p_row) - p_row[own speaker]
 *   loss    (1)       float64 mean of the row terms
 * fp32 sums in orders fixed by (M, C); permuting the speakers permutes sim, p1, p2 bit for bit; the fold is float64 in an
 * order fixed by N*M; no atomics.  A centroid of zero norm gives NaN, as in the reference.
 * PK_ESHAPE: N < 2, M < 2 (the exclusive centroid divides by M - 1) or C < 1.  PK_EUNSUPPORTED (never truncated): N > 4096,
 * C > 2048, N*M > 2^20 or N*M*N > 2^28. */
int pk_spk_ge2e(pk_spk* h, const float* embeds, int32_t N, int32_t M, int32_t C, float* sim, float* p1, float* p2,
                double* row_nll, double* loss);
/* out[u] = a[u] . b[u] / (max(|a[u]|, 1e-12) max(|b[u]|, 1e-12)) for u < U: the cosine similarity of two (U, C) float32 arrays
 * of embeddings, all three on the DEVICE (how close a cloned voice is to its reference).  PK_ESHAPE: U < 1 or C < 1. */
int pk_spk_cosine(pk_spk* h, const float* a, const float* b, int32_t U, int32_t C, float* out);
void pk_spk_destroy(pk_spk* h);

/* ------------------------------------------------- STFT / mel / log features */
/* parakeet/modules/audio.py STFT (:74-215) + MelScale (:218-229); host twin
 * parakeet/data/get_feats.py LogMelFBank (:20-88). */
typedef struct {
    int32_t n_fft;        /* 1024 */
    int32_t hop_length;   /* 256 */
    int32_t center;       /* 1: reflect-pad n_fft/2 on both sides (:175-179) */
    int32_t power;        /* 0: magnitude sqrt(re^2+im^2) (:202-215); 1: power (:198-200) */
    int32_t n_mels;       /* 80; 0 = no mel stage */
    int32_t log_base;     /* 0 none, 10 (TTS features, get_feats.py:84-85), 2 = natural log (:86-87) */
    float log_floor;      /* 1e-10 (np.clip a_min, :83) */
} pk_mel_cfg;

/* window: n_fft floats (scipy.signal.get_window(..., fftbins=True), centre-padded to n_fft, :133-141);
 * mel_basis: (n_mels, 1 + n_fft/2) row-major (librosa.filters.mel), may be NULL if n_mels == 0. */
int pk_mel_create(pk_ctx* ctx, const pk_mel_cfg* cfg, const float* window, const float* mel_basis,
                  pk_mel** out);
/* frames = 1 + (n_samples + 2*pad - n_fft) / hop  (:103-105). */
int pk_mel_num_frames(pk_mel* h, int32_t n_samples, int32_t* frames);
/* wav: packed samples, lens (B) host.  out is packed by utterance, time-major:
 * what 0: (frames, 2*n_bin) real | imag (STFT.forward); 1: (frames, n_bin) magnitude / power;
 * 2: (frames, n_mels) mel (then log if configured);
 * 3: (frames, 1) frame energy sqrt(max(sum_k |X_k|^2, log_floor)) (get_feats.py Energy :196-203), reduced in the kernel
 *    that reads the frame's spectrum. */
int pk_mel_run(pk_mel* h, const float* wav, const int32_t* lens, int32_t B, float* out,
               int32_t what, int32_t flags);
/* How the handle transforms its frames.  PK_TRANSFORM_DENSE (the default): the product with the windowed DFT basis.
 * PK_TRANSFORM_FFT: the radix FFT of csrc/rfft.hip -- frame * window in fp32, then the transform; the re | im rows of
 * what 0 - 3 come from it, every later stage is the same.  Timeline rows that belong to no frame are skipped for what 0.
 * n_fft must be a power of two from 32 to 4096, else PK_EUNSUPPORTED (the handle keeps its transform); another value of
 * `transform`: PK_EINVAL. */
#define PK_TRANSFORM_DENSE 0
#define PK_TRANSFORM_FFT 1
int pk_mel_set_transform(pk_mel* h, int32_t transform);
void pk_mel_destroy(pk_mel* h);
/* The radix FFT as a primitive (csrc/rfft.hip, plan and rounding count in csrc/pk_rfft.h): numpy.fft.rfft / irfft of
 * `rows` rows of n real points, n a power of two from 32 to 4096 (pk_rfft_supported: 1, else 0; another n:
 * PK_EUNSUPPORTED).  x (rows, n) and out (rows, n + 2) = re (n/2 + 1) | im (n/2 + 1) per row, the layout of
 * pk_mel_run(what = 0); pk_op_irfft reads that layout and writes (rows, n), ignoring im(DC) and im(Nyquist) as numpy does
 * and scaling by 1/n.  DEVICE pointers, 8-byte aligned; enqueued on the context's stream (the first call for an n uploads
 * its twiddle table and synchronises).  One workgroup transforms pk_rfft_tile_rows(n) whole rows; a row's result is the
 * same bits wherever it stands in a batch. */
int pk_rfft_supported(int32_t n);
int pk_rfft_tile_rows(int32_t n, int32_t* rows);
int pk_op_rfft(pk_ctx* ctx, const float* x, int64_t rows, int32_t n, float* out);
int pk_op_irfft(pk_ctx* ctx, const float* spec, int64_t rows, int32_t n, float* out);
/* Token averages of frame-level features (get_feats.py _average_by_duration :141-153, :205-214):
 * out[t] = mean(x[cum[t-1]:cum[t]]) over the frames of token t, 0 for a token of 0 frames; spans are cut at `frames`
 * like a numpy slice.  x: DEVICE (frames, C); durations: HOST (T), >= 0; out: DEVICE (T, C).  Synchronises. */
int pk_op_average_by_duration(pk_ctx* ctx, const float* x, int64_t frames, int32_t C, const int64_t* durations,
                              int32_t T, float* out);

/* ------------------------------------------------ inverse STFT / Griffin-Lim */
/* parakeet/audio/audio.py AudioProcessor.istft (:86-93) = librosa.istft: every frame is irfft(D[:, f], n_fft) * window
 * (the imaginary parts of DC and Nyquist are ignored, as numpy.fft.irfft does), frames are overlap-added at stride
 * hop_length, every sample is divided by the overlap-added window^2 where that envelope exceeds FLT_MIN and left
 * undivided elsewhere, and with center n_fft/2 samples are cut from both ends.
 * Limits as for the STFT: n_fft a multiple of 16 (and <= 16384), hop_length a multiple of 4, else PK_EUNSUPPORTED.
 * The overlap-add is a gather in ascending frame order without atomics and shares nothing between utterances: the
 * samples of an utterance are bit-identical in any batch and at any position in it. */
typedef struct pk_istft pk_istft;
typedef struct {
    int32_t n_fft;
    int32_t hop_length;
    int32_t center;       /* 1: the spectra come from a centred STFT; n_fft/2 samples are trimmed from both ends */
} pk_istft_cfg;
/* window: n_fft floats, centre-padded to n_fft as for pk_mel_create. */
int pk_istft_create(pk_ctx* ctx, const pk_istft_cfg* cfg, const float* window, pk_istft** out);
/* samples returned for `frames` >= 1 frames: hop * (frames - 1) with center, else n_fft + hop * (frames - 1). */
int pk_istft_num_samples(pk_istft* h, int32_t frames, int32_t* n);
/* spec: (sum(frames), 2*n_bin) real | imag, packed by utterance and time-major -- what pk_mel_run(what = 0) writes;
 * frames (B) host, each >= 1 (else PK_EINVAL); wav_out packed by utterance, pk_istft_num_samples floats each.
 * flags: PK_HOST_IO if spec / wav_out are host pointers (then synchronous). */
int pk_istft_run(pk_istft* h, const float* spec, const int32_t* frames, int32_t B, float* wav_out, int32_t flags);
/* Fast Griffin-Lim (librosa.griffinlim; Perraudin, Balazs, Sondergaard 2013): phases for a magnitude spectrogram.
 *   angles = initial phases; rebuilt = 0
 *   n_iter times: previous = rebuilt; rebuilt = STFT(ISTFT(mag * angles));
 *                 angles = rebuilt - momentum / (1 + momentum) * previous; angles /= |angles| + 1e-16
 *   wav_out = ISTFT(mag * angles)
 * momentum = 0 is the classic algorithm; n_iter = 0 is pk_istft_run of mag * angles, bit for bit.  All iterations are
 * enqueued on the context's stream without a host synchronisation in between.
 *   stft    a pk_mel handle of the same context with the same n_fft, hop_length, center (and window); its packed basis
 *           runs the forward transform.  A mismatch -> PK_EINVAL.
 *   mag     (sum(frames), n_bin) packed like spec;  frames (B) host.  With center and n_iter > 0 an utterance needs
 *           hop * (frames - 1) > n_fft / 2 (the forward STFT reflect-pads it), else PK_EINVAL.
 *   angles  (sum(frames), 2*n_bin) cos | sin, or NULL: exp(2 pi i u) with u = word * 2^-32, word (bin & 3) of the
 *           Philox4x32-10 block with counter (frame index inside its utterance, bin >> 2, 0, 0x474C5048 "GLPH") and
 *           key seeds[b] -- a seed reproduces an utterance exactly in any batch (the contract of the dropout stream).
 *   seeds   (B) host, NULL = all 0; unused when angles are given
 *   n_iter >= 0, 0 <= momentum < 1, else PK_EINVAL.
 * flags: PK_HOST_IO if mag / angles / wav_out are host pointers (then synchronous). */
int pk_gl_run(pk_istft* h, pk_mel* stft, const float* mag, const int32_t* frames, int32_t B, int32_t n_iter,
              float momentum, const uint64_t* seeds, const float* angles, float* wav_out, int32_t flags);
/* Test taps of the last pk_gl_run, copied to HOST as (sum(frames), 2*n_bin) re | im, n = that many floats (else PK_ESHAPE):
 * 0 = the spectrum the last iteration's forward STFT rebuilt (PK_ESTATE after n_iter = 0), 1 = the last iterate
 * mag * angles, the spectrum the returned waveform is the ISTFT of. */
int pk_gl_debug_read(pk_istft* h, int32_t what, float* out, int64_t n);
/* PK_TRANSFORM_DENSE (default) or PK_TRANSFORM_FFT, as pk_mel_set_transform: under FFT every frame is the inverse radix
 * FFT of its re | im row (read where the caller left it), times the window; overlap-add and everything else are the
 * same kernels.  pk_gl_run needs both handles on the same transform (else PK_EINVAL) and then runs both directions of its
 * loop on it; n_iter = 0 stays pk_istft_run of mag * angles, bit for bit, on that transform. */
int pk_istft_set_transform(pk_istft* h, int32_t transform);
void pk_istft_destroy(pk_istft* h);

/* ------------------------------------------------------------- resampling */
/* Rational-ratio resampling of ragged batches as a polyphase FIR (csrc/resample.hip); the reference's recipes begin with
 * librosa.load(path, sr=fs) (examples/fastspeech2/preprocess.py:54-55), whose filter this is NOT: the filter is whatever
 * table the caller passes (parakeet_amd/audio.py resample_filter builds a Kaiser-windowed sinc).
 *   y[n] = sum_k table[(n * down) mod up][k] * x[floor(n * down / up) - (taps - 1) / 2 + k],   n = 0 ... ceil(N * up / down) - 1
 * with x = 0 outside 0 ... N - 1: row p of `table` is the phase p / up, and tap k of a row multiplies the input sample
 * k - (taps - 1) / 2 (integer division) away from the output's input base.  Taps are accumulated in ascending k with one fp32
 * FMA each (the kernel also adds 0 * x for up to ceil(down / up) samples on either side of an output's taps: nothing for
 * finite x, but an Inf or NaN sample reaches outputs that far beyond the filter's support too).  up = down = 1 is a plain FIR filter with the one row of the table (a caller that wants equal rates to be the
 * identity does not call the engine: parakeet_amd.audio.Resample).
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): 1 <= up, down <= 4096; 1 <= taps <= 8192;
 * up * taps <= 4 Mi coefficients. */
typedef struct pk_resample pk_resample;
typedef struct {
    int32_t up;           /* L: target rate / gcd */
    int32_t down;         /* M: source rate / gcd */
    int32_t taps;         /* T: taps per phase */
} pk_resample_cfg;
/* table: HOST, (up, taps) row-major, copied. */
int pk_resample_create(pk_ctx* ctx, const pk_resample_cfg* cfg, const float* table, pk_resample** out);
/* n_out = ceil(n_in * up / down), 0 <= n_in < 2^31 (else PK_EINVAL). */
int pk_resample_out_len(pk_resample* h, int64_t n_in, int64_t* n_out);
/* Outputs per workgroup.  Tiles start at utterance-relative multiples of it (a multiple of up). */
int pk_resample_tile_samples(pk_resample* h, int32_t* tile);
/* wav: packed samples of B utterances, lens (B, host) >= 1 each; out: packed, pk_resample_out_len floats per utterance.
 * An utterance's output is bit-identical alone, in any batch and at any position in it; the samples of its neighbours in the
 * packed buffer are never read.
 * PK_EINVAL: NULL pointer, B <= 0, an empty utterance.
 * flags: PK_HOST_IO if wav / out are host pointers (then synchronous). */
int pk_resample_run(pk_resample* h, const float* wav, const int32_t* lens, int32_t B, float* out, int32_t flags);
void pk_resample_destroy(pk_resample* h);

/* ------------------------------------------------------------------ pitch */
/* Frame-level f0 of ragged batches (csrc/pitch.hip) behind the reference's Pitch (parakeet/data/get_feats.py:91-164), which
 * calls pyworld's DIO + StoneMask.  This is NOT that estimator: it is the project's own, defined in DESIGN 4.5e (the
 * difference function, cumulative-mean normalisation, absolute threshold and parabolic refinement of YIN):
 *   frames = n / hop + 1;  frame i reads L = win + tau_max samples from s = i * hop - L / 2, zeros outside the utterance
 *   d(tau)  = sum_{j < win} (x[s + j] - x[s + j + tau])^2,  tau = 1 ... tau_max   (fp32, j ascending, one chain per lag)
 *   d'(tau) = d(tau) * tau / c(tau) with c(tau) = d(1) + ... + d(tau), 1 where c(tau) is not > 0;  d'(0) = 1
 *   tau0 = the smallest tau in [tau_min, tau_max - 1] with d'(tau) < threshold; none: lag 0, f0 0 (unvoiced)
 *   tau* = tau0, then + 1 while tau* + 1 <= tau_max - 1 and d'(tau* + 1) < d'(tau*)
 *   a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1);  delta = (a - c) / (2 (a - 2 b + c)) if a >= b, c >= b and
 *   a - 2 b + c > 0, else 0;  f0 = sr / (tau* + delta)  (the refinement in float64 on the fp32 d', rounded once)
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): 2 <= tau_min <= tau_max - 2, tau_max <= 960,
 * 1 <= win <= 2 * tau_max, 1 <= hop <= 16384.  PK_EINVAL: sr < 1, a threshold that is not a number. */
typedef struct pk_pitch pk_pitch;
typedef struct {
    int32_t sr;
    int32_t hop;
    int32_t tau_min;
    int32_t tau_max;
    int32_t win;
    float threshold;
} pk_pitch_cfg;
int pk_pitch_create(pk_ctx* ctx, const pk_pitch_cfg* cfg, pk_pitch** out);
/* frames = n_samples / hop + 1, 0 <= n_samples < 2^31 (else PK_EINVAL). */
int pk_pitch_frames(pk_pitch* h, int64_t n_samples, int32_t* frames);
/* Frames per workgroup.  Tiles start at utterance-relative multiples of it. */
int pk_pitch_tile_frames(pk_pitch* h, int32_t* tile);
/* wav: packed samples of B utterances, lens (B, host) >= 1 each.  Packed by utterance: f0_out one float per frame (0 for an
 * unvoiced frame), lag_out (NULL: not wanted) one int32 tau* per frame (0 for unvoiced), cmnd_out (NULL: not wanted)
 * tau_max + 1 floats d'(0 ... tau_max) per frame.  A frame depends on its own samples only: an utterance's result is
 * bit-identical alone, in any batch and at any position in it; its neighbours in the packed buffer are never read.
 * PK_EINVAL: NULL h / wav / lens / f0_out, B <= 0, an empty utterance.
 * flags: PK_HOST_IO if wav and the outputs are host pointers (then synchronous). */
int pk_pitch_run(pk_pitch* h, const float* wav, const int32_t* lens, int32_t B, float* f0_out, int32_t* lag_out,
                 float* cmnd_out, int32_t flags);
/* A second decision stage behind the same d': Viterbi tracking over per-frame candidates ("Viterbi tracking over
 * candidates"; this project's own design, like the estimator).  pk_pitch_run's results are not touched by it.
 *   candidates of a frame: the lags tau in [tau_min, tau_max - 1] with d'(tau) < d'(tau - 1), d'(tau) <= d'(tau + 1) and
 *     d'(tau) < theta_c (fp32 comparisons); the K smallest by (d', tau) are kept and stored by ascending tau, an empty slot
 *     has lag 0 and cost +inf
 *   states of a frame: the K slots (observation cost: d' of the slot, as float64) and "unvoiced" (unvoiced_cost)
 *   transitions: slot to slot lambda * |T[tau_s] - T[tau_p]|, T a float64 table of log2(tau) made on the host; unvoiced to
 *     unvoiced 0; voiced to unvoiced or back switch_cost
 *   D_0[s] = obs_0[s];  D_i[s] = min_p (D_(i-1)[p] + tr(p, s)) + obs_i[s] in float64, added in that order, the product not
 *     contracted into the sum; a tie goes to the smaller p (unvoiced is the last state), slots of cost +inf are skipped; the
 *     path ends in the smallest s of minimal D, which is the score; a frame's lag is its state's, 0 for unvoiced, and f0 is
 *     refined as pk_pitch_run refines it.
 * PK_EINVAL: K outside 1 ... 8, a threshold that is not a number, a cost that is negative, infinite or not a number. */
typedef struct {
    int32_t K;               /* candidates kept per frame */
    float theta_c;           /* candidate threshold */
    double lambda;           /* cost of one octave between consecutive voiced frames */
    double unvoiced_cost;    /* observation cost of the unvoiced state (parakeet_amd.audio.Pitch passes its threshold) */
    double switch_cost;      /* voiced <-> unvoiced */
} pk_pitch_track_cfg;
/* wav, lens, B, flags: as pk_pitch_run.  Every output may be NULL; packed by utterance: f0_out one float and lag_out one int32
 * per frame (0 for an unvoiced frame), score_out one double per utterance, cand_lag_out / cand_cost_out K values per frame.
 * An utterance's results are bit-identical alone, in any batch and at any position in it.
 * PK_EINVAL: NULL h / wav / lens / cfg, B <= 0, an empty utterance, and the configuration's (above).
 * PK_EUNSUPPORTED: an utterance of more than 2^22 frames. */
int pk_pitch_track_run(pk_pitch* h, const float* wav, const int32_t* lens, int32_t B, const pk_pitch_track_cfg* cfg, float* f0_out,
                       int32_t* lag_out, double* score_out, int32_t* cand_lag_out, float* cand_cost_out, int32_t flags);
/* The same on d' rows of the caller: cmnd holds tau_max + 1 floats per frame, packed by track; frames (B, host) >= 1 each.
 * Rows that pk_pitch_run wrote give what pk_pitch_track_run gives, bit for bit.  Values in the rows that are not numbers are
 * never candidates; negative values order as numbers do.  PK_EINVAL / PK_EUNSUPPORTED as above (an empty track: PK_EINVAL). */
int pk_pitch_track_from_cmnd(pk_pitch* h, const float* cmnd, const int32_t* frames, int32_t B, const pk_pitch_track_cfg* cfg,
                             float* f0_out, int32_t* lag_out, double* score_out, int32_t* cand_lag_out, float* cand_cost_out,
                             int32_t flags);
/* Named integer options (results do not change):
 *   "track_lds_frames"  1 ... 4096 (default 4096): tracks of more frames keep the tracker's backpointers in a global workspace,
 *                       not in LDS */
int pk_pitch_set_option(pk_pitch* h, const char* key, int64_t value);
void pk_pitch_destroy(pk_pitch* h);
/* Pitch._convert_to_continuous_f0 (get_feats.py:99-119) and the log step of _calculate_f0 (:136-138) for B packed f0
 * tracks, from any estimator: frames before the first / after the last non-zero value take that value, a zero frame i
 * between non-zero neighbours a < i < b takes f(a) + (f(b) - f(a)) (i - a) / (b - a) (float64, rounded once), a track
 * without a non-zero value is returned as it is; with bit 0 of log_flag every non-zero result v becomes log(v) (float64,
 * rounded once); bit 1 leaves the filling out (the reference's use_continuous_f0 = False: the log step alone).
 * f0, out: DEVICE, packed, out must not overlap f0; frames (B, host) >= 1 each, of any length.  Synchronises.
 * PK_EINVAL: NULL pointer, B <= 0, an empty track, a log_flag outside 0 ... 3. */
int pk_op_continuous_f0(pk_ctx* ctx, const float* f0, const int32_t* frames, int32_t B, int32_t log_flag, float* out);

/* ------------------------------------------------------- silence trimming */
/* Framed power, the frame test of librosa.effects.trim / split, the reference's trim_long_silences
 * (examples/ge2e/audio_processor.py:53-107) after its voice detector, and peak normalisation, for ragged batches
 * (csrc/trim.hip).  Every pointer below is a DEVICE pointer unless it says host; packed means utterance after
 * utterance.  An utterance's results are bit-identical alone, in any batch and at any position in it; its neighbours in the
 * packed buffer are never read.
 *   frames(N) = 1 + (N + 2 pad - Lf) / hop, pad = Lf / 2 (pad_mode 1, 2) or 0 (pad_mode 0; no frame when N < Lf);
 *   P[i] = (1 / Lf) sum_{j < Lf} x~[i hop - pad + j]^2, x~ continued by reflection without repeating the edge (pad_mode 1,
 *   needs N > Lf / 2) or by zeros (pad_mode 2); summed in fp32 in the order csrc/pk_trim.h states;
 *   frame i is non-silent iff max(1e-10, P[i]) > max(1e-10, max_i P) * factor (in float64; factor = 10^(-top_db / 10));
 *   start = first non-silent frame * hop, end = min(N, (last non-silent frame + 1) * hop); none: (0, 0).
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): 1 <= hop <= Lf <= 16384; window <= 16384;
 * 1 <= avg_width <= 64; 0 <= max_silence <= 64.
 * PK_EINVAL: NULL pointer, B <= 0, an empty utterance, an unknown pad_mode, reflect padding of N <= Lf / 2 samples. */
typedef struct pk_trim pk_trim;
int pk_trim_create(pk_ctx* ctx, pk_trim** out);       /* workspaces only: one handle serves every parameter set */
void pk_trim_destroy(pk_trim* h);
int pk_trim_num_frames(int64_t n_samples, int32_t frame_length, int32_t hop, int32_t pad_mode, int64_t* frames);
/* Frames per workgroup of the power kernel.  Tiles start at utterance-relative multiples of it. */
int pk_trim_tile_frames(int32_t frame_length, int32_t hop, int32_t* tile);
/* lens (B, host).  power_out (NULL: a workspace): packed P, one float per frame; with rms != 0 its square root (then no
 * flags and no bounds).  flags_out (NULL: not wanted): packed, one byte per frame, 1 = non-silent.  bounds_out (NULL: not
 * wanted): (B, 2) int32 (start, end).  Two launches, no read-back. */
int pk_trim_run(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t frame_length, int32_t hop,
                int32_t pad_mode, double factor, int32_t rms, float* power_out, uint8_t* flags_out, int32_t* bounds_out);
/* trim_long_silences up to the gather.  n_w = N / window windows per utterance (the tail is dropped; n_w = 0 is allowed).
 * Voice flags: voice_flags (packed, one byte per window) if not NULL -- from any detector --, else this project's energy
 * detector, NOT webrtcvad: Q[k] = the window's power (frames with Lf = hop = window, no padding) and
 * flag[k] iff Q[k] > max(max_k Q * rel, floor_power) (float64).  Then, as the reference: c = the set flags in
 * [k - (W - 1) / 2, k + W / 2] inside the utterance, mask[k] iff 2 c > W (its moving average rounded half to even);
 * keep[k] = any mask[k - (L - 1 - L / 2) ... k + L / 2], L = max_silence + 1 (its binary_dilation with ones(L)).
 * pos_out: packed int32 per window: the window's index among the kept ones of its utterance, -1 if dropped.  kept (B, HOST):
 * kept windows per utterance; the call synchronises to deliver it.  power_out / flags_out (NULL: not wanted): Q and the
 * voice flags, packed.  wav may be NULL when voice_flags is given. */
int pk_vad_mask(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t window, int32_t avg_width,
                int32_t max_silence, const uint8_t* voice_flags, double rel, double floor_power, float* power_out,
                uint8_t* flags_out, int32_t* pos_out, int32_t* kept);
/* out: packed, kept[b] * window samples per utterance: its kept windows in order.  pos, kept: as pk_vad_mask left them. */
int pk_vad_gather(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, int32_t window, const int32_t* pos,
                  const int32_t* kept, float* out);
/* out = y / max|y| per utterance, one correctly rounded division per sample; an utterance whose max|y| is below the smallest
 * normal float is copied as it is.  out is packed like wav and must not overlap it. */
int pk_peak_normalize(pk_trim* h, const float* wav, const int32_t* lens, int32_t B, float* out);

/* ------------------------------------------- multi-resolution STFT distance */
/* parakeet/modules/stft_loss.py: what MultiResolutionSTFTLoss (:163-219) needs of two signals, reduced on the device.
 * A handle holds R resolutions.  n_fft must be a multiple of 16 (else PK_EUNSUPPORTED); hop_length is ANY integer >= 1
 * (a handle of its own: pk_mel_* and pk_istft_* keep their hop % 4 == 0 limit). */
typedef struct pk_stftd pk_stftd;
typedef struct {
    int32_t n_fft;        /* 1024 */
    int32_t hop_length;   /* 120 */
    int32_t center;       /* 1: reflect-pad n_fft/2 on both sides */
} pk_stftd_resolution;
typedef struct {
    int32_t n_res;        /* R */
    float power_floor;    /* 1e-7: X = sqrt(max(re^2 + im^2, power_floor))  (stft_loss.py:66) */
    float log_floor;      /* 1e-7: ln(max(X, log_floor))                    (:98, :117-118) */
} pk_stftd_cfg;
/* res: R entries; windows: the R windows one after the other, n_fft floats each, centre-padded as for pk_mel_create. */
int pk_stftd_create(pk_ctx* ctx, const pk_stftd_cfg* cfg, const pk_stftd_resolution* res, const float* windows,
                    pk_stftd** out);
/* frames of resolution r = 1 + (n_samples + 2*pad - n_fft) / hop. */
int pk_stftd_num_frames(pk_stftd* h, int32_t r, int32_t n_samples, int32_t* frames);
/* x (predicted), y (ground truth): packed samples of B utterances with the same lens (B, host).
 * sums_out (B, R, 3) float64, per utterance and resolution over its frames x n_bin entries:
 *   [0] sum (Y - X)^2    [1] sum Y^2    [2] sum |ln max(Y, log_floor) - ln max(X, log_floor)|
 * (terms in fp32, a frame's terms added in fp32, an utterance's frames in fp64).  No magnitude is stored.  An utterance's
 * sums are bit-identical in any batch and at any position in it.
 * PK_EINVAL: NULL pointer, B <= 0, an utterance with lens <= n_fft/2 of a centred resolution (reflect padding).
 * flags: PK_HOST_IO if x / y / sums_out are host pointers (then synchronous). */
int pk_stftd_run(pk_stftd* h, const float* x, const float* y, const int32_t* lens, int32_t B, double* sums_out,
                 int32_t flags);
/* The floored magnitude of resolution r: out packed (sum(frames), n_bin), by utterance and time-major.  Errors and flags
 * as pk_stftd_run. */
int pk_stftd_magnitude(pk_stftd* h, int32_t r, const float* wav, const int32_t* lens, int32_t B, float* out,
                       int32_t flags);
void pk_stftd_destroy(pk_stftd* h);

/* ------------------------------------------- Parallel WaveGAN discriminator */
/* parakeet/models/parallel_wavegan/parallel_wavegan.py PWGDiscriminator.forward :523-630 for ragged batches, and the sums the
 * evaluator's MSE terms are formed of (parallel_wavegan_updater.py:192-223).  layers - 1 blocks of Conv1D(kernel_size,
 * dilation d_i, zero padding (kernel_size - 1) / 2 * d_i) + LeakyReLU(negative_slope), d_0 = 1 and d_i = i for
 * dilation_factor 1, else dilation_factor^i; then Conv1D(conv_channels -> 1, kernel_size), no activation.  Inference only.
 * The whole stack is one kernel (csrc/pwg_disc.hip): a window of 256 samples (128 above 64 channels) of one utterance stays
 * in LDS through all layers; its middle, window - 2 * halo samples, is the output tile.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): in_channels = out_channels = 1; kernel_size odd, 1 ... 9;
 * layers 3 ... 16 (the reference cannot run 2); conv_channels a multiple of 16 in 16 ... 128; dilation_factor >= 1 with the
 * receptive field per side, halo = (kernel_size - 1) / 2 * (sum of the d_i + 1), AT MOST 112 SAMPLES up to 64 channels and
 * 48 above (the released recipes: 38). */
typedef struct pk_pwgd pk_pwgd;
typedef struct {
    int32_t in_channels;      /* 1 */
    int32_t out_channels;     /* 1 */
    int32_t kernel_size;      /* 3 */
    int32_t layers;           /* 10 */
    int32_t conv_channels;    /* 64 */
    int32_t dilation_factor;  /* 1 */
    float negative_slope;     /* 0.2 */
    int32_t bias;             /* 1 */
} pk_pwgd_cfg;
int pk_pwgd_create(pk_ctx* ctx, const pk_pwgd_cfg* cfg, pk_pwgd** out);
/* name: the reference's state-dict key, "conv_layers.{2i}.weight" (or .weight_g / .weight_v, folded at finalize) and
 * "conv_layers.{2i}.bias" for block i = 0 ... layers - 1 (the last one is the output conv). */
int pk_pwgd_set_param(pk_pwgd* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int pk_pwgd_finalize(pk_pwgd* h);
/* PK_PWG_MATH_F16X3 (default; the activations' block scale is measured per window and layer, the weights carry one exponent
 * per tensor) or PK_PWG_MATH_F32.  Block 0 and the output conv are fp32 FMAs in both.  PK_PWG_MATH_BF16X3: PK_EUNSUPPORTED. */
int pk_pwgd_set_math(pk_pwgd* h, int32_t mode);
/* The kernel's output tile and the receptive field per side (samples).  Tiles start at utterance-relative multiples of tile. */
int pk_pwgd_tile_samples(pk_pwgd* h, int32_t* tile, int32_t* halo);
/* wav: packed samples of B utterances, lens (B, host) >= 1 each.
 * logits_out: NULL, or packed (sum lens) logits.  With NULL no logit is written to memory.
 * sums_out: NULL, or (B, 2) float64: [0] sum (p - 1)^2, [1] sum p^2 over the utterance's logits p (terms in fp32, a tile's
 * terms added in fp32, an utterance's tiles in fp64 in a fixed order; no atomics).
 * An utterance's logits and sums are bit-identical alone, in any batch and at any position in it.
 * PK_EINVAL: NULL wav / lens, B <= 0, an empty utterance.  PK_ESTATE before pk_pwgd_finalize.
 * flags: PK_HOST_IO if wav / logits_out / sums_out are host pointers (then synchronous). */
int pk_pwgd_run(pk_pwgd* h, const float* wav, const int32_t* lens, int32_t B, float* logits_out, double* sums_out,
                int32_t flags);
/* on != 0: every pk_pwgd_run keeps a copy of its input for pk_pwgd_debug_read (off by default: it costs a copy). */
int pk_pwgd_set_debug(pk_pwgd* h, int32_t on);
/* Test tap: the activation after block `layer` (0 ... layers - 2, after its LeakyReLU) of utterance b of the last run, copied
 * to HOST as (conv_channels, lens[b]) channel-major, n_floats = that many (else PK_ESHAPE).  Runs the stack again over that
 * utterance in the handle's current math.  PK_ESTATE without a run under pk_pwgd_set_debug(h, 1). */
int pk_pwgd_debug_read(pk_pwgd* h, int32_t layer, int32_t b, float* host_out, int64_t n_floats);
void pk_pwgd_destroy(pk_pwgd* h);

/* ------------------------------------------------------- HiFi-GAN generator */
/* The generator of HiFi-GAN (Kong et al. 2020), restated from the paper with the module layout of the usual
 * HiFiGANGenerator; NEITHER THE PARAMETER NAMES NOR THE OUTPUT SLOPE BELOW COULD BE CHECKED AGAINST A REAL CHECKPOINT.
 * With ch_i = channels >> i and a_s = LeakyReLU(s):
 *   x = Conv1D(in_channels -> channels, kernel_size)(mel)                                            "input_conv"
 *   per stage i (scale s_i): x = Conv1DTranspose(ch_i -> ch_(i+1), 2 s_i, stride s_i, padding s_i / 2 + s_i % 2,
 *                                output_padding s_i % 2)(a_slope(x))                                 "upsamples.{i}.1"
 *     per residual block j (kernel k_j), y = x, for its n-th dilation d:
 *       t = Conv1D(k_j, dilation d)(a_slope(y))                                                      "blocks.{i nb + j}.convs1.{n}.1"
 *       use_additional_convs: t = Conv1D(k_j)(a_slope(t))                                            "blocks.{i nb + j}.convs2.{n}.1"
 *       y = t + y
 *     x = (sum_j y_j) / nb
 *   wav = tanh(Conv1D(ch_last -> 1, kernel_size)(a_0.01(x)))                                         "output_conv.1"
 * Every convolution zero-pads its own input at the two ends of the utterance.  Weights: Conv1D (C_out, C_in, k),
 * Conv1DTranspose (C_in, C_out, k); ".weight", or ".weight_g" / ".weight_v" folded at finalize (norm over all axes but 0).
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): in_channels 1 ... 512, out_channels 1; kernel_size odd
 * 3 ... 11; 1 ... 6 stages with scales 2 ... 16 and upsample_kernel_sizes[i] == 2 * upsample_scales[i]; hop 4 ... 1024; every
 * ch_i a multiple of 8 in 8 ... 512; 1 ... 4 residual blocks with odd kernels 3 ... 11 and 1 ... 4 dilations each,
 * (k - 1) / 2 * d <= 64; bias = 1. */
#define PK_HFG_MAX_STAGES 6
#define PK_HFG_MAX_BLOCKS 4
#define PK_HFG_MAX_DILS 4
typedef struct pk_hfg pk_hfg;
typedef struct {
    int32_t in_channels;                  /* 80 */
    int32_t out_channels;                 /* 1 */
    int32_t channels;                     /* 512 */
    int32_t kernel_size;                  /* 7 */
    int32_t n_upsample;                   /* 4 */
    int32_t upsample_scales[PK_HFG_MAX_STAGES];         /* 8, 8, 2, 2 */
    int32_t upsample_kernel_sizes[PK_HFG_MAX_STAGES];   /* 16, 16, 4, 4 */
    int32_t n_blocks;                     /* 3 */
    int32_t resblock_kernel_sizes[PK_HFG_MAX_BLOCKS];   /* 3, 7, 11 */
    int32_t n_dilations[PK_HFG_MAX_BLOCKS];             /* 3, 3, 3 */
    int32_t resblock_dilations[PK_HFG_MAX_BLOCKS][PK_HFG_MAX_DILS];   /* 1, 3, 5 each */
    int32_t use_additional_convs;         /* 1 */
    int32_t bias;                         /* 1 */
    float negative_slope;                 /* 0.1 */
} pk_hfg_cfg;
int pk_hfg_create(pk_ctx* ctx, const pk_hfg_cfg* cfg, pk_hfg** out);
int pk_hfg_set_param(pk_hfg* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int pk_hfg_finalize(pk_hfg* h);
/* PK_PWG_MATH_F16X3 (default; the activations' block scale is one exponent per utterance and layer input, measured by the
 * layer that produced it; the weights carry one exponent per tensor) or PK_PWG_MATH_F32.  PK_PWG_MATH_BF16X3: PK_EUNSUPPORTED. */
int pk_hfg_set_math(pk_hfg* h, int32_t mode);
/* ZScore statistics of in_channels elements, applied ((x - mu) / sigma) only by calls with PK_APPLY_NORMALIZER; NULL, NULL: none. */
int pk_hfg_set_normalizer(pk_hfg* h, const float* mu, const float* sigma, int32_t n);
/* mel: packed (sum frames, in_channels); frames (B, host) >= 1 each; wav_out: packed (sum frames * hop).  An utterance's
 * samples are bit-identical alone, in any batch and at any position in it.  The workspace is sized per call from the frame
 * counts; a call that would need more than 16 GiB of activations returns PK_ENOMEM (split the batch; chunking one long
 * utterance is not implemented).  flags: PK_APPLY_NORMALIZER, PK_HOST_IO (mel and wav_out are host pointers; synchronous). */
int pk_hfg_infer(pk_hfg* h, const float* mel, const int32_t* frames, int32_t B, float* wav_out, int32_t flags);
/* Test tap: the output of stage `stage` (0 ... n_upsample - 1) after its block mean, of utterance b of the last
 * pk_hfg_infer, copied to HOST as (channels >> (stage + 1), frames[b] * scales up to the stage) channel-major; n_floats =
 * that many (else PK_ESHAPE).  Runs the stack again over that utterance in the handle's current math.  PK_ESTATE without
 * a pk_hfg_infer since the parameters were last set. */
int pk_hfg_debug_read(pk_hfg* h, int32_t stage, int32_t b, float* host_out, int64_t n_floats);
/* Test tap of one convolution: what launch `launch` of the stack wrote for utterance b of the last pk_hfg_infer, to HOST as
 * (C_out, positions) channel-major.  Launches in order: input_conv; per stage the transposed convolution, then per residual
 * block and dilation convs1 (t), with use_additional_convs convs2 (t + y; the block's last one writes the running block
 * mean instead); the output convolution's wav is what pk_hfg_infer returns.  Runs the stack again up to that launch. */
int pk_hfg_debug_conv(pk_hfg* h, int32_t launch, int32_t b, float* host_out, int64_t n_floats);
void pk_hfg_destroy(pk_hfg* h);

/* ------------------------------------------------------- pseudo-QMF bank */
/* The analysis / synthesis filter bank of multi-band MelGAN (csrc/pk_pqmf.h defines the arithmetic, tests/pqmf_ref.py
 * restates it).  Filters, computed once on the host in float64 and rounded once to float32; K = subbands, n = 0 ... taps,
 * c = n - taps / 2:
 *   proto[n]       = sin(pi cutoff c) / (pi c) * kaiser(taps + 1, beta)[n]; the centre tap is cutoff
 *   analysis_k[n]  = 2 proto[n] cos((2 k + 1) pi / (2 K) c + (-1)^k pi / 4)
 *   synthesis_k[n] = the same with - (-1)^k pi / 4
 * analysis: wav (L) -> bands (K, floor(L / K)), the zero-padded (taps / 2 each side) correlation with analysis_k taken at
 * every K-th sample.  synthesis: bands (K, M) -> wav (K M): K - 1 zeros between samples, scaled by K, zero-padded by
 * taps / 2, correlated with synthesis_k and summed over k; evaluated in its polyphase form, ceil((taps + 1) / K) products
 * per band and sample at most.  Every product is one fmaf in a fixed order (pk_pqmf.h): a sample is bit-identical alone,
 * in any batch and at any position in it.  No atomics.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): subbands 2 ... 16, taps even 4 ... 254, cutoff_ratio in
 * (0, 0.5), beta 0 ... 700 (beyond, I0(beta) is no float64). */
typedef struct pk_pqmf pk_pqmf;
typedef struct {
    int32_t subbands;                     /* 4 */
    int32_t taps;                         /* 62 */
    float cutoff_ratio;                   /* 0.142 */
    float beta;                           /* 9.0 */
} pk_pqmf_cfg;
int pk_pqmf_create(pk_ctx* ctx, const pk_pqmf_cfg* cfg, pk_pqmf** out);
/* The float32 filters to HOST, (subbands, taps + 1) each; n_floats = subbands * (taps + 1) (else PK_ESHAPE). */
int pk_pqmf_filters(pk_pqmf* q, float* analysis_out, float* synthesis_out, int64_t n_floats);
/* wav: packed (sum lens); lens (B, host) >= subbands each (else PK_EINVAL); bands_out: per utterance a (subbands,
 * floor(lens[b] / subbands)) channel-major block, the blocks packed in order.  flags: PK_HOST_IO (synchronous). */
int pk_pqmf_analysis(pk_pqmf* q, const float* wav, const int32_t* lens, int32_t B, float* bands_out, int32_t flags);
/* bands: per utterance a (subbands, band_lens[b]) channel-major block, packed; band_lens (B, host) >= 1 each; wav_out:
 * packed (sum band_lens * subbands).  flags: PK_HOST_IO (synchronous). */
int pk_pqmf_synthesis(pk_pqmf* q, const float* bands, const int32_t* band_lens, int32_t B, float* wav_out, int32_t flags);
void pk_pqmf_destroy(pk_pqmf* q);

/* ------------------------------------------------------- MelGAN / multi-band MelGAN generator */
/* The generator of MelGAN (Kumar et al. 2019) and of multi-band MelGAN (Yang et al. 2020) with the module layout of the
 * usual MelGANGenerator, as recalled; NEITHER THE PARAMETER NAMES NOR THIS LAYOUT COULD BE CHECKED AGAINST A RELEASED
 * CHECKPOINT.  With ch_i = channels >> i, a = LeakyReLU(negative_slope), S = stacks, R = ReflectionPad1d:
 *   x = Conv1D(in_channels -> channels, kernel_size)(R((kernel_size - 1) / 2)(mel))                    "melgan.1"
 *   per stage i (scale s_i), q_i = 2 + i (2 + S):
 *     x = Conv1DTranspose(ch_i -> ch_(i+1), 2 s_i, stride s_i, padding s_i / 2 + s_i % 2,
 *                         output_padding s_i % 2)(a(x))                                                "melgan.{q_i + 1}"
 *     per stack j = 0 ... S - 1, d = stack_kernel_size ^ j:
 *       t = Conv1D(k = stack_kernel_size, dilation d)(R((k - 1) / 2 d)(a(x)))                          "melgan.{q_i + 2 + j}.stack.2"
 *       x = Conv1D(1x1)(a(t)) + Conv1D(1x1)(x)                   "melgan.{q_i + 2 + j}.stack.4", "melgan.{q_i + 2 + j}.skip_layer"
 *   y = Conv1D(ch_last -> out_channels, kernel_size)(R(...)(a(x)))                                     "melgan.{2 + n (2 + S) + 2}"
 *   y = tanh(y) with use_final_nonlinear_activation
 * Weights: Conv1D (C_out, C_in, k), Conv1DTranspose (C_in, C_out, k); ".weight", or ".weight_g" / ".weight_v" folded at
 * finalize (norm over all axes but 0).  A stack is three launches of the HiFi-GAN convolution kernel: the dilated
 * convolution under the reflecting boundary rule, the skip convolution (slope 1: LeakyReLU is the identity), the 1x1
 * convolution of a(t) whose epilogue adds the skip.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): in_channels 1 ... 512; out_channels 1 ... 16; kernel_size
 * odd 3 ... 11; 1 ... 6 stages with scales 2 ... 16; every ch_i a multiple of 8 in 8 ... 512; stacks 1 ... 6,
 * stack_kernel_size odd 3 ... 7 with (k - 1) / 2 * k^(S - 1) <= 64; bias = 1; reflection padding, no causal convolutions.
 * Reflection needs its pad smaller than the length it pads at every padded convolution: pk_mgan_min_frames is the
 * smallest admissible frame count (4 for the defaults); pk_mgan_infer returns PK_EINVAL naming it for a shorter utterance. */
#define PK_MGAN_MAX_STAGES 6
typedef struct pk_mgan pk_mgan;
typedef struct {
    int32_t in_channels;                  /* 80 */
    int32_t out_channels;                 /* 1; multi-band: 4 */
    int32_t channels;                     /* 512 */
    int32_t kernel_size;                  /* 7 */
    int32_t n_upsample;                   /* 4 */
    int32_t upsample_scales[PK_MGAN_MAX_STAGES];   /* 8, 8, 2, 2 */
    int32_t stacks;                       /* 3 */
    int32_t stack_kernel_size;            /* 3 */
    int32_t bias;                         /* 1 */
    int32_t use_final_nonlinear_activation;   /* 1 */
    float negative_slope;                 /* 0.2 */
} pk_mgan_cfg;
int pk_mgan_create(pk_ctx* ctx, const pk_mgan_cfg* cfg, pk_mgan** out);
int pk_mgan_set_param(pk_mgan* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
int pk_mgan_finalize(pk_mgan* h);
/* PK_PWG_MATH_F16X3 (default; block scales as pk_hfg_set_math) or PK_PWG_MATH_F32.  PK_PWG_MATH_BF16X3: PK_EUNSUPPORTED. */
int pk_mgan_set_math(pk_mgan* h, int32_t mode);
int pk_mgan_set_normalizer(pk_mgan* h, const float* mu, const float* sigma, int32_t n);
/* The smallest frame count pk_mgan_infer accepts for an utterance. */
int32_t pk_mgan_min_frames(const pk_mgan* h);
/* Attach a synthesis bank (NULL: detach): requires subbands == out_channels (else PK_EINVAL).  pk_mgan_infer then writes
 * the full-band waveform, frames * hop * subbands samples per utterance, straight from the sub-band buffer.  The bank must
 * outlive the attachment and live on the same context. */
int pk_mgan_set_pqmf(pk_mgan* h, pk_pqmf* pqmf);
/* mel: packed (sum frames, in_channels); frames (B, host) >= pk_mgan_min_frames each (else PK_EINVAL).  out: per utterance
 * (out_channels, frames[b] * hop) channel-major, the blocks packed in order -- the waveform for out_channels = 1 -- or,
 * with a bank attached, the packed full-band waveform (sum frames * hop * subbands).  An utterance's samples are
 * bit-identical alone, in any batch and at any position in it.  Plain launches, no atomics.  The workspace is sized per
 * call; a call that would need more than 16 GiB of activations returns PK_ENOMEM (split the batch; chunking one long
 * utterance is not implemented).  flags: PK_APPLY_NORMALIZER, PK_HOST_IO (mel and out are host pointers; synchronous). */
int pk_mgan_infer(pk_mgan* h, const float* mel, const int32_t* frames, int32_t B, float* out, int32_t flags);
/* Test tap: the output of stage `stage` (0 ... n_upsample - 1, after its last stack) of utterance b of the last
 * pk_mgan_infer, to HOST as (channels >> (stage + 1), frames[b] * scales up to the stage); n_floats = that many (else
 * PK_ESHAPE).  Runs the stack again over that utterance.  PK_ESTATE without a pk_mgan_infer since the parameters were set. */
int pk_mgan_debug_read(pk_mgan* h, int32_t stage, int32_t b, float* host_out, int64_t n_floats);
/* Test tap of one launch, to HOST as (C_out, positions).  Launches in order: the input convolution; per stage the transposed
 * convolution, then per stack t, the skip convolution, x'; last the output convolution (out_channels, frames[b] * hop): the
 * sub-bands, also when a bank is attached. */
int pk_mgan_debug_conv(pk_mgan* h, int32_t launch, int32_t b, float* host_out, int64_t n_floats);
void pk_mgan_destroy(pk_mgan* h);

/* ------------------------------------------------- masked L1 + SSIM of mel pairs */
/* The two spectrogram terms of the SpeedySpeech evaluator (speedyspeech_updater.py:119-140) in one pass over both
 * images, and parakeet/modules/ssim.py:21-61 (channel = 1) as a metric of its own.
 * pred, target: packed rows (sum lens, W), W in [1, 1024].  lens: HOST (B) valid rows of each pair; padded_lens: HOST (B)
 * >= lens, or NULL = lens: the rows of each pair's SSIM map.  Rows at or past lens[b] read as zero in both images
 * (decoded * spec_mask, target * spec_mask); borders are zero-padded by window_size / 2 on all four sides.  The window is
 * the reference's: gaussian of sigma 1.5, exp in double, rounded to fp32, divided by its fp32 sum; C1 = 1e-4, C2 = 9e-4.
 * window_size must be odd and >= 1 (PK_EINVAL; an even window changes the map's size in the reference) and at most 33
 * (PK_EUNSUPPORTED).
 * sums_out (B, 2) double: sum |pred - target| over the lens[b] x W valid entries; sum of the SSIM map over its
 * padded_lens[b] x W entries.  A pair's two sums are the same bits alone and in any batch.
 * ssim_map_out: NULL, or packed (sum padded_lens, W): the map itself.  PK_HOST_IO honoured for all data pointers. */
int pk_mel_loss_run(pk_ctx* ctx, const float* pred, const float* target, const int32_t* lens, const int32_t* padded_lens,
                    int32_t B, int32_t W, int32_t window_size, double* sums_out, float* ssim_map_out, int32_t flags);

/* ------------------------------------- per-utterance sums of the acoustic models' criteria */
/* seq_loss.hip: what FastSpeech2Loss, TransformerTTSLoss, GuidedAttentionLoss and Tacotron2Loss reduce, left as float64
 * sums per utterance; the host forms the means (mask modes, weights, normalisations).  Common to the three calls: lengths
 * and offsets are HOST arrays, offsets and strides count floats, PK_HOST_IO is honoured for all data pointers (then
 * synchronous); every term enters a float64 accumulator at once and partial sums are combined in a fixed order (no
 * atomics), so an utterance's sums are the same bits alone, in any batch, at any position and in either layout.
 * PK_EINVAL: NULL argument, B <= 0, a negative length or offset.
 *
 * pk_pair_loss_run: pair b is rows[b] x W entries of pred and of target, W in [1, 8192] (above: PK_EUNSUPPORTED), row r at
 * pred + pred_offs[b] + r * pred_stride (target likewise).  pred_offs / target_offs NULL: the pairs follow one another
 * (packed; the stride must then be 0 or W).  A stride of 0 means W.  A padded (B, Lmax, W) rectangle is offs[b] =
 * b * Lmax * W with stride W; a column block of a wider tensor is a larger stride.  rows[b] may be 0.
 * sums_out (B, 2) double: sum |p - t| (difference in fp32), sum (p - t)^2 (the fp32 difference squared exactly). */
int pk_pair_loss_run(pk_ctx* ctx, const float* pred, const float* target, const int64_t* pred_offs, const int64_t* target_offs,
                     int64_t pred_stride, int64_t target_stride, const int32_t* rows, int32_t B, int32_t W, double* sums_out,
                     int32_t flags);
/* Paddle's binary_cross_entropy_with_logits term, (1 - y) x + (1 + (pos_weight - 1) y) (log1p(exp(-|x|)) + max(-x, 0)),
 * evaluated in float64 in this form (finite for any finite logit) and summed over row b's lens[b] entries at
 * logits + logit_offs[b], labels + label_offs[b] (NULL: packed).  labels are floats.  pos_weight must be finite and >= 0
 * (PK_EINVAL); 1 is the unweighted loss.  sums_out (B) double. */
int pk_bce_logits_run(pk_ctx* ctx, const float* logits, const float* labels, const int64_t* logit_offs,
                      const int64_t* label_offs, const int32_t* lens, int32_t B, float pos_weight, double* sums_out,
                      int32_t flags);
/* Guided attention (Tachibana et al. 2017): utterance b owns maps[b] attention maps of rows[b] x cols[b] entries, map g's
 * row s at att + offs[b] + g * map_stride + s * row_stride.  offs NULL: everything contiguous, utterance after utterance
 * (both strides must be 0).  row_stride 0 means cols[b], map_stride 0 means rows[b] * row stride; a zero-padded
 * (B, G, Smax, Tmax) tensor is offs[b] = b * G * Smax * Tmax, map_stride = Smax * Tmax, row_stride = Tmax.
 * The guide W[s, t] = 1 - exp(-(t / cols[b] - s / rows[b])^2 / (2 sigma^2)) is formed in fp32 in the reference's order (two
 * quotients, difference, square, division by fp32(2 sigma^2), expf) once per tile and never stored; it is
 * GuidedAttentionLoss._make_guided_attention_mask (rows = olen, cols = ilen) and attention_guide (rows = dec_len, cols =
 * enc_len) alike.  sums_out (B, 2) double: sum over g, s, t of W * A (product exact), sum of A.
 * PK_EINVAL: sigma <= 0 or not finite, an utterance without a map, row or column, a stride below the extent it spans.
 * PK_EUNSUPPORTED: more than 4096 maps in an utterance. */
int pk_guided_attn_run(pk_ctx* ctx, const float* att, const int64_t* offs, int64_t map_stride, int64_t row_stride,
                       const int32_t* maps, const int32_t* rows, const int32_t* cols, int32_t B, double sigma, double* sums_out,
                       int32_t flags);

/* --------------------------------------- durations from a teacher's attention */
/* Monotonic alignment search (the best monotonic path through a score matrix, the dynamic programme of Glow-TTS's
 * maximum_path) and the focus rate of attention maps (FastSpeech, 3.3) for ragged batches (csrc/align.hip).
 * The definition is this project's own (csrc/pk_align.h states it in full); it is NOT the Montreal Forced Aligner.  Data
 * pointers are DEVICE pointers; offs, rows, cols, maps are HOST arrays; offsets and strides count floats.  An utterance's
 * results are the same bits alone, in any batch and at any position in it; its neighbours in a packed buffer are never read.
 *
 * pk_mas_run: utterance b is rows[b] (decoder steps S) x cols[b] (tokens T) entries, row s at scores_or_att + offs[b] +
 * s * row_stride.  offs NULL: the utterances follow one another (row_stride must be 0); row_stride 0 means cols[b]; a padded
 * (B, Smax, Tmax) tensor is offs[b] = b * Smax * Tmax, row_stride = Tmax.  mode 0: the entries are the scores v; mode 1: they
 * are attention weights A and v = logf(A < eps ? eps : A) (eps > 0 and finite).  Q(0, 0) = v(0, 0), Q(s, t) = v(s, t) +
 * max(Q(s - 1, t), Q(s - 1, t - 1)) in float64 for t <= s, -inf otherwise; the path ends in (S - 1, T - 1) and at row s >= 1
 * stays in its column t iff Q(s - 1, t) >= Q(s - 1, t - 1).
 *   durations_out  packed int32, sum cols: rows of the path per token, each >= 1, summing to rows[b];
 *   path_out       NULL, or packed int32, sum rows: the path's column at every row;
 *   score_out      NULL, or (B) double: Q(S - 1, T - 1);
 *   status_out     NULL, or (B) int32: 1 if a v(s, t) with t <= s is not finite (that utterance's durations and path are then
 *                  unspecified), else 0;
 *   scores_out     NULL, or (mode 1 only) packed float, sum rows * cols, contiguous: the v the search used.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit): cols <= 1024, rows <= 16384.
 * PK_EINVAL: NULL ctx / input / rows / cols / durations_out, B <= 0, an empty utterance, cols[b] > rows[b], a stride below
 * the columns, an unknown mode, eps that is not positive and finite. */
int pk_mas_run(pk_ctx* ctx, const float* scores_or_att, const int64_t* offs, int64_t row_stride, const int32_t* rows,
               const int32_t* cols, int32_t B, int32_t mode, float eps, int32_t* durations_out, int32_t* path_out,
               double* score_out, int32_t* status_out, float* scores_out);
/* The 32-bit decision words of an utterance that stay in LDS; an utterance has rows * 2 * ceil(cols / 64) of them and keeps
 * them in a global workspace when that is more. */
int pk_mas_lds_words(int32_t* words);
/* Focus rate F = (1 / S) sum_s max_t A[s, t] of every map; the layout is pk_guided_attn_run's (utterance b owns maps[b]
 * maps of rows[b] x cols[b], map g's row s at att + offs[b] + g * map_stride + s * row_stride; zero strides and NULL
 * offsets as there).  The maximum is exact, the sum float64 in the fixed order csrc/pk_align.h states.  rates_out: packed
 * double, sum maps.  PK_EINVAL as for pk_guided_attn_run; PK_EUNSUPPORTED: more than 2^30 maps in a call. */
int pk_focus_rate_run(pk_ctx* ctx, const float* att, const int64_t* offs, int64_t map_stride, int64_t row_stride,
                      const int32_t* maps, const int32_t* rows, const int32_t* cols, int32_t B, double* rates_out);

/* ------------------------------------- dynamic time warping and its path statistics */
/* Unconstrained dynamic time warping of ragged batches and float64 sums along the path (csrc/dtw.hip): what
 * mel-cepstral distortion and log-F0 RMSE of free-running synthesis are taken along (parakeet_amd/metrics.py).  The
 * definition is this project's own (csrc/pk_dtw.h states it in full: squared Euclidean local cost, no band, no slope weights).
 * Data pointers are DEVICE pointers; offs_*, rows, cols are HOST arrays; offsets and strides count floats.  A pair's results
 * are the same bits alone, in any batch and at any position in it; its neighbours in a packed buffer and the padding of a
 * padded tensor are never read.
 *
 * pk_dtw_run: pair b has rows[b] = N rows (frames of x) and cols[b] = M columns (frames of y).
 *   mode 0: x_or_cost holds the float32 cost matrices, row i of pair b at x_or_cost + offs_x[b] + i * stride_x (stride 0:
 *           cols[b]; offs_x NULL: the matrices follow one another); y, offs_y, stride_y, D, k0, k1 are not looked at.
 *   mode 1: x_or_cost holds the (N, D) features x, y the (M, D) features y (row strides 0: D; NULL offsets: the pairs follow
 *           one another); c(i, j) = (float) sum_{k0 <= k < k1} ((double)x[i, k] - (double)y[j, k])^2, summed ascending with
 *           separate float64 operations, formed on the device into a workspace of the context (pk_dtw_cost_cap).
 *   Q(0, 0) = c(0, 0), Q(i, j) = c(i, j) + min(Q(i - 1, j - 1), Q(i - 1, j), Q(i, j - 1)) in float64; the predecessor is the
 *   smallest, ties to the diagonal, then to (i - 1, j).
 *   ix_out, iy_out  packed int32, N + M - 1 entries per pair (pair b starts at the sum of those before it): the path in
 *                   forward order from (0, 0) to (N - 1, M - 1); entries from the path's length on are never written;
 *   len_out         (B) int32: the path's length P, max(N, M) <= P <= N + M - 1;
 *   cost_out        NULL, or (B) double: Q(N - 1, M - 1);
 *   status_out      NULL, or (B) int32: 1 if a c(i, j) is not finite (that pair's path is then unspecified), else 0.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit; nothing is launched): rows, cols <= 4096, D <= 128,
 * B <= 65535.  PK_EINVAL: a NULL pointer that is needed, B <= 0, an empty pair, a column range outside [0, D), a stride
 * below the extent it spans or without offsets, a negative offset, an unknown mode. */
int pk_dtw_run(pk_ctx* ctx, int32_t mode, const float* x_or_cost, const float* y, const int64_t* offs_x, const int64_t* offs_y,
               int64_t stride_x, int64_t stride_y, int32_t D, int32_t k0, int32_t k1, const int32_t* rows, const int32_t* cols,
               int32_t B, int32_t* ix_out, int32_t* iy_out, int32_t* len_out, double* cost_out, int32_t* status_out);
/* Feature mode's cost matrices alone (the kernel pk_dtw_run launches): cost_out packed float, sum rows * cols, contiguous. */
int pk_dtw_cost(pk_ctx* ctx, const float* x, const float* y, const int64_t* offs_x, const int64_t* offs_y, int64_t stride_x,
                int64_t stride_y, int32_t D, int32_t k0, int32_t k1, const int32_t* rows, const int32_t* cols, int32_t B,
                float* cost_out);
/* The 32-bit decision words of a pair that stay in LDS; a pair has cols * ceil(rows / R) of them, R = the smallest of 1, 2,
 * 4, 8, 16 with 64 R >= rows (16 beyond), and keeps them in a global workspace when that is more. */
int pk_dtw_lds_words(int32_t* words);
/* The cap in bytes on feature mode's cost workspace (256 MiB unless set; process-wide): set_bytes 0 leaves it, bytes_out may
 * be NULL.  A call whose matrices exceed it runs in several launches over consecutive pairs; a launch holds at least one
 * pair, whatever the cap. */
int pk_dtw_cost_cap(int64_t set_bytes, int64_t* bytes_out);
/* Sums along paths.  ix, iy, len: as pk_dtw_run writes them for the same rows, cols (DEVICE pointers).  x, y and the column
 * range as in mode 1.  mask_x, mask_y: NULL, or packed uint8 (sum rows / sum cols).  s_p is the float64 sum of step p.
 *   sums_out    (B, 2) double: sum s_p, sum sqrt(s_p) over the steps whose two masks are set (all steps without masks), in
 *               the fixed order csrc/pk_dtw.h states; no atomics;
 *   counts_out  (B, 4) int64: the steps with (mask_x, mask_y) set = (1, 1), (1, 0), (0, 1), (0, 0);
 *   status_out  NULL, or (B) int32: 2 if len or a path entry lies outside the pair (such steps are left out), else 0. */
int pk_dtw_path_stats(pk_ctx* ctx, const int32_t* ix, const int32_t* iy, const int32_t* len, const float* x, const float* y,
                      const int64_t* offs_x, const int64_t* offs_y, int64_t stride_x, int64_t stride_y, int32_t D, int32_t k0,
                      int32_t k1, const int32_t* rows, const int32_t* cols, int32_t B, const uint8_t* mask_x,
                      const uint8_t* mask_y, double* sums_out, int64_t* counts_out, int32_t* status_out);

/* ------------------------------------------------- edit distance and its alignment */
/* The edit (Levenshtein) distance of ragged batches of token sequences and the alignment it comes from (csrc/edit.hip,
 * DESIGN 4.7c): what word, character and phone error rates are counted from (parakeet_amd/utils/error_rate.py).  csrc/pk_edit.h
 * states the definition in full.  ref, hyp and the outputs are DEVICE pointers; offs_*, n, m are HOST arrays; offsets count
 * ids.  A pair's results are the same bits alone, in any batch and at any position in it; its neighbours in a packed buffer
 * and the padding of a padded tensor are never read.
 *
 * pk_edit_run: pair b has n[b] = N >= 0 int32 ids at ref + offs_ref[b] and m[b] = M >= 0 at hyp + offs_hyp[b] (NULL offsets: the
 * pairs follow one another).  Any int32 value is an id; only equality is used.
 *   D(i, 0) = i, D(0, j) = j, D(i, j) = D(i - 1, j - 1) if ref[i - 1] == hyp[j - 1], else 1 + min(D(i - 1, j - 1), D(i - 1, j),
 *   D(i, j - 1)); the walk back from (N, M) takes a hit on equal ids, else the first of substitution (i - 1, j - 1), deletion
 *   (i - 1, j), insertion (i, j - 1) whose value is D(i, j) - 1; insertions in row 0, deletions in column 0.
 *   mode 0: dist_out alone is written (counts_out, ops_out, len_out are not looked at): no ops are kept, nothing is walked.
 *   mode 1: all four.
 *   dist_out    (B) int32: D(N, M);
 *   counts_out  (B, 4) int32: hits, substitutions, deletions, insertions;
 *   ops_out     packed uint8, N + M entries per pair (pair b starts at the sum of those before it): the ops in forward order,
 *               0 hit, 1 substitution, 2 deletion, 3 insertion; entries from len_out[b] on are never written;
 *   len_out     (B) int32: their number P, max(N, M) <= P <= N + M.
 * Envelope (else PK_EUNSUPPORTED, the message names the limit; nothing is launched): n, m <= 4096, B <= 65535.  PK_EINVAL: a
 * NULL pointer that is needed, B <= 0, a negative length or offset, an unknown mode. */
int pk_edit_run(pk_ctx* ctx, const int32_t* ref, const int32_t* hyp, const int64_t* offs_ref, const int64_t* offs_hyp,
                const int32_t* n, const int32_t* m, int32_t B, int32_t mode, int32_t* dist_out, int32_t* counts_out,
                uint8_t* ops_out, int32_t* len_out);
/* The 32-bit op words of a pair that stay in LDS (mode 1); a pair has m * ceil(n / R) of them, R = the smallest of 1, 2, 4,
 * 8, 16 with 64 R >= n (16 beyond), and keeps them in a global workspace when that is more. */
int pk_edit_lds_words(int32_t* words);

/* ------------------------------------- short-time objective intelligibility (STOI, ESTOI) */
/* STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of time-aligned pairs of signals at 10 kHz, ragged batches in one
 * call (csrc/stoi.hip).  csrc/pk_stoi.h states the definition in full; it is this project's own restatement of
 * the papers (NOT pystoi's or MATLAB's code), and fewer than 30 spectrum frames give NaN with segments = 0, not 1e-5.
 * Signals, bands and outputs are DEVICE pointers unless said otherwise; offs is a HOST array of B + 1 ascending sample
 * offsets, utterance b being the samples [offs[b], offs[b + 1]) of the packed signals (empty utterances are allowed).  No
 * atomics, fixed summation orders: an utterance's results are the same bits alone, in any batch and at any position in it.
 * Every call uploads its table (and synchronises for that), enqueues its kernels on the context's stream and reads nothing
 * back.  Envelope (else PK_EUNSUPPORTED, nothing is launched): B <= 65535, 2^30 samples per utterance, 2^29 frames per call.
 * PK_EINVAL: a NULL pointer that is needed, B <= 0, descending or negative offsets, a negative frame count. */
typedef struct pk_stoi_result {
    double d;           /* the score; NaN where segments == 0 */
    int32_t segments;   /* S = (kept - 1) - 29, at least 0 */
    int32_t kept;       /* frames of the clean signal that survive silent-frame removal */
    int32_t frames;     /* F(L), the frames of the signal */
    int32_t reserved;
} pk_stoi_result;
/* The whole pipeline: silent-frame removal decided on `clean`, both signals rebuilt, band magnitudes, segment correlations
 * (extended != 0: ESTOI).  result_out: (B) records.  The kept-frame counts never reach the host. */
int pk_stoi_run(pk_ctx* ctx, const float* clean, const float* degraded, const int64_t* offs, int32_t B, int32_t extended,
                pk_stoi_result* result_out);
/* Stage 1 alone.  With F_b = F(offs[b + 1] - offs[b]) and frames packed utterance after utterance (sum F_b entries):
 *   energy_out  NULL, or float: e_i = 20 log10(||w x_i|| + EPS) in dB (the float64 value the test used, rounded);
 *   keep_out    NULL, or uint8: 1 iff the frame is kept;
 *   index_out   NULL, or int32: the first kept_out[b] entries of utterance b's stretch are its kept frames, ascending;
 *   kept_out    (B) int32. */
int pk_stoi_mask(pk_ctx* ctx, const float* clean, const int64_t* offs, int32_t B, float* energy_out, uint8_t* keep_out,
                 int32_t* index_out, int32_t* kept_out);
/* Stage 3 alone on given signals: every frame of x (F_b per utterance, nothing removed, nothing rebuilt) times w, zero-padded
 * to 512, transformed on the radix FFT; bands_out: packed float (sum F_b, 15). */
int pk_stoi_bands(pk_ctx* ctx, const float* x, const int64_t* offs, int32_t B, float* bands_out);
/* Stage 4 alone: bands_x, bands_y packed float (sum frames[b], 15), frames HOST (B).  d_out (B) double, segments_out NULL or
 * (B) int32: frames[b] - 29, at least 0. */
int pk_stoi_segments(pk_ctx* ctx, const float* bands_x, const float* bands_y, const int32_t* frames, int32_t B,
                     int32_t extended, double* d_out, int32_t* segments_out);
/* HOST only: F(L) of the frame rule; the bins [lo[j], hi[j]) of the 15 one-third-octave bands. */
int pk_stoi_num_frames(int64_t n_samples, int64_t* frames);
int pk_stoi_band_edges(int32_t* lo, int32_t* hi);

/* ------------------------------------- recursive filters, gated loudness (BS.1770, mono), gain */
/* Cascades of second-order sections over ragged batches in float64, and programme loudness on the same passes (csrc/iir.hip,
 * DESIGN 4.5h).  csrc/pk_iir.h states the recurrence, the plan of 256-sample chunks and every summation order; the loudness
 * measure is this project's own restatement of ITU-R BS.1770-4 for one channel (NOT pyloudnorm, NOT libebur128), with blocks
 * on a 100 ms sample grid.  x, y and the result arrays are DEVICE pointers; lens and gains are HOST arrays of B entries,
 * utterance b being lens[b] samples of the packed signal behind utterance b - 1 (empty utterances are allowed and produce
 * nothing).  No atomics, fixed orders: an utterance's results are the same bits alone, in any batch and at any position.
 * Every call uploads its table (and synchronises for that), enqueues its kernels on the context's stream and reads nothing
 * back.  Envelope (else PK_EUNSUPPORTED, nothing is launched): B <= 65535, 2^30 samples per utterance, at most 8 sections,
 * sr a multiple of 10 in 8 000 ... 192 000.  PK_EINVAL: a NULL pointer, B <= 0, a negative length, fewer than one section,
 * a0 != 1, a coefficient that is not finite. */
typedef struct pk_iir pk_iir;
/* sos: HOST (n_sections, 6) double, scipy's rows (b0, b1, b2, a0, a1, a2) with a0 == 1.  The transition matrix of a chunk is
 * computed on the device here, once. */
int pk_iir_create(pk_ctx* ctx, const double* sos, int32_t n_sections, pk_iir** out);
void pk_iir_destroy(pk_iir* h);
/* The transition matrix P, (2 n_sections, 2 n_sections) row-major, into a HOST array. */
int pk_iir_transition(pk_iir* h, double* P_out);
/* y = the filter of x, the state zero at every utterance's first sample; one float32 rounding per sample. */
int pk_iir_run(pk_iir* h, const float* x, const int32_t* lens, int32_t B, float* y);
/* Gated loudness of x at rate sr, h holding the weighting filter (K-weighting for BS.1770).  Per utterance: mean_out (B)
 * double, the mean power of the blocks both gates keep (0 where none); rel_out (B) double, the relative threshold as a power
 * (0 where the absolute gate keeps nothing); peak_out (B) float, max|x|; counts_out (B, 3) int32: the blocks both gates keep,
 * those the absolute gate keeps, all blocks.  LUFS = -0.691 + 10 log10(mean) is the host's to form. */
int pk_loudness_run(pk_iir* h, const float* x, const int32_t* lens, int32_t B, int32_t sr, double* mean_out, double* rel_out,
                    float* peak_out, int32_t* counts_out);
/* y = x * gains[b] over utterance b, one rounding (y may be x). */
int pk_gain_run(pk_ctx* ctx, const float* x, const int32_t* lens, int32_t B, const float* gains, float* y);

/* ------------------------------------------------------- phase vocoder (time stretching, pitch shifting) */
/* A spectrogram re-timed by a rate (csrc/pvoc.hip): what librosa 0.8's phase_vocoder(D, rate, hop_length)
 * computes, as this project restates it in float64 without any transcendental function (csrc/pk_pvoc.h states every
 * operation; the accumulated phase is a running product of unit phasors, hop_length has no effect).  NOT librosa's bits, no
 * phase locking.  spec and out are DEVICE pointers to packed ragged rows of 2 * n_bin floats, re | im, the layout of
 * pk_mel_run(what = 0) and pk_istft_run: utterance b is frames[b] rows of spec behind utterance b - 1, and T_b rows of out,
 * T_b = ceil(frames[b] / rates[b]) in float64 (pk_pvoc_num_frames).  frames and rates are HOST arrays of B entries, one rate
 * per utterance.  No atomics, no reduction: an utterance's bytes are the same alone, in any batch and at any position.  The
 * call uploads its table (and synchronises for that), enqueues one kernel on the context's stream and reads nothing back.
 * PK_EINVAL: a NULL pointer, B <= 0, n_bin < 1, a frame count below 1, a rate that is not finite or not > 0, T_b >= 2^31.
 * PK_EUNSUPPORTED: B > 65535. */
int pk_pvoc_num_frames(int64_t frames, double rate, int64_t* out_frames);
int pk_pvoc_run(pk_ctx* ctx, const float* spec, const int32_t* frames, int32_t B, int32_t n_bin, const double* rates, float* out);

/* ------------------------------------------------------- feature statistics */
/* Streaming mean / variance of ragged feature matrices (csrc/stats.hip): what the reference's
 * utils/compute_statistics.py takes from scikit-learn's StandardScaler.partial_fit.  A handle is an accumulator over feature
 * dimension D with the state
 *   n (int64 rows), K (D float32, the shift), S1[c] = sum (x[r, c] - K[c]), S2[c] = sum (x[r, c] - K[c])^2 (float64).
 * K is fixed once: the shift given to pk_stats_reset, else the first row the accumulator ever sees.  Differences, squares
 * and additions are single IEEE float64 operations in THE ORDER csrc/pk_stats.h states (row tiles anchored at the
 * utterance's first row, a fixed lane map, a fixed tree; utterances added left to right): an utterance's sums are the same
 * bytes alone and in any batch, a corpus gives the same state bytes in any split into updates at utterance boundaries.  No
 * atomics.  NaN and Inf propagate.  mean = K + S1 / n, var = max(S2 - S1^2 / n, 0) / n are formed by the caller.
 * Envelope (else PK_EUNSUPPORTED, before any launch): 1 <= D <= 1024; lens[b] <= 2^31 - 1; at most 2^24 tiles per update.
 * PK_EINVAL: NULL handle / lens, B <= 0, a negative length, NULL rows with rows to read, unknown flags. */
typedef struct pk_stats pk_stats;
#define PK_STATS_MOMENTS_ONLY 1   /* pk_stats_update: write moments_out only; n, K, S1, S2 stay (PK_ESTATE while K is open) */
int pk_stats_create(pk_ctx* ctx, int32_t D, pk_stats** out);
void pk_stats_destroy(pk_stats* h);
/* n = 0, S1 = S2 = 0; shift (HOST, D floats) fixes K, NULL leaves it open for the first row.  Synchronises. */
int pk_stats_reset(pk_stats* h, const float* shift);
/* Rows per tile for dimension D (HOST out); tiles start at utterance-relative multiples of it. */
int pk_stats_tile_rows(int32_t D, int32_t* rows);
/* rows: DEVICE, packed (sum lens, D) float32, utterance after utterance.  lens: HOST (B) int64; 0 is allowed and adds
 * nothing.  moments_out: NULL, or DEVICE (B, 2 D) float64: utterance b's S1 | S2 about K.  The state becomes
 * S + U_0 + U_1 + ... + U_{B-1}, added in that order.  Three launches, no read-back. */
int pk_stats_update(pk_stats* h, const float* rows, const int64_t* lens, int32_t B, double* moments_out, int32_t flags);
/* The state through HOST buffers (any may be NULL): n, have_shift (0 while K is open), shift (D floats), s1, s2 (D doubles
 * each).  pk_stats_get synchronises the stream first; pk_stats_set with shift NULL (only with n = 0) leaves K open. */
int pk_stats_get(pk_stats* h, int64_t* n, int32_t* have_shift, float* shift, double* s1, double* s2);
int pk_stats_set(pk_stats* h, int64_t n, const float* shift, const double* s1, const double* s2);

/* ------------------------------------------------------------ normal noise */
/* Standard-normal floats on the device: out[i] for i in [0, n), a pure function of (seed, offset + i).
 * Replaces the paddle.randn calls of PWGGenerator.inference (parallel_wavegan.py:515-516) and
 * ConditionalWaveFlow.infer (waveflow.py:801) for callers that hold no device RNG of their own.
 * Philox4x32-10 (Salmon et al., SC'11; key = seed, counter = (offset + i) / 4) -> 4 x uint32 ->
 * Box-Muller on pairs: u1 = (a + 1) * 2^-32 in (0, 1], u2 = b * 2^-32,
 * r = sqrt(-2 ln u1), (z0, z1) = r * (cos, sin)(2 pi u2).  offset must be a multiple of 4.
 * flags: PK_HOST_IO if out is a host pointer (then synchronous). */
int pk_randn(pk_ctx* ctx, float* out, int64_t n, uint64_t seed, uint64_t offset, int32_t flags);
/* Seed of the internal generator used when pk_pwg_infer / pk_wf_infer get noise == NULL (default 0);
 * every such call consumes a fresh, non-overlapping range of the stream. */
int pk_pwg_set_seed(pk_pwg* h, uint64_t seed);
int pk_wf_set_seed(pk_wf* h, uint64_t seed);

/* ------------------------------------------ generic primitives (parakeet/modules) */
/* sinusoid_position_encoding (positional_encoding.py:20-39) -> out (num_positions, feature_size), device. */
int pk_op_sinusoid_position_encoding(pk_ctx* ctx, int32_t num_positions, int32_t feature_size,
                                     float omega, int32_t start_pos, float* out);
/* scaled_dot_product_attention (attention.py:22-58), eval mode (no dropout).  q (B,Tq,d), k (B,Tk,d),
 * v (B,Tk,dv) device; mask float (zeros = padding, adds (1-mask)*-1e9) or NULL, mask_mode 0: (B,1,Tk),
 * 1: (B,Tq,Tk), 2: (1,Tq,Tk).  out (B,Tq,dv); weights (B,Tq,Tk) or NULL. */
int pk_op_scaled_dot_product_attention(pk_ctx* ctx, const float* q, const float* k, const float* v,
                                       const float* mask, int32_t mask_mode, int32_t B, int32_t Tq,
                                       int32_t Tk, int32_t d, int32_t dv, float* out, float* weights);
/* Conv1dBatchNorm.forward (conv.py:186-260) in eval mode, data_format "NLC", stride 1, symmetric
 * padding: x (B,T,Cin) device -> y (B, T+2*pad-k+1, Cout) device.  weight [Cout][Cin][k], bias [Cout] or
 * NULL, BatchNorm1D weight/bias/_mean/_variance [Cout] (all four or none) are HOST pointers.
 * Supported range: 1 <= k <= 12, Cin a multiple of 16 (else PK_EUNSUPPORTED), any pad >= 0 with
 * T + 2*pad - k + 1 >= 1 (else PK_ESHAPE) -- pad may exceed k - 1, the output is then longer than the input
 * by rows that see only zeros and hold the folded bias, as with paddle.nn.Conv1D.
 * Synchronous (weights are packed per call). */
int pk_op_conv1d_batchnorm_nlc(pk_ctx* ctx, const float* x, int32_t B, int32_t T, int32_t Cin,
                               int32_t Cout, int32_t k, int32_t pad, const float* weight,
                               const float* bias, const float* bn_weight, const float* bn_bias,
                               const float* bn_mean, const float* bn_var, float eps, float* y);

/* Conv1dCell.add_input (modules/conv.py:166-183): one step of a causal dilated Conv1D used as a cell.  buffer DEVICE
 * (B, Cin, r), r = 1 + (k - 1) * dilation, zeros before the first step (initialize_buffer :129-139), shifted by one
 * step and fed x_t DEVICE (B, Cin) here; weight DEVICE [Cout][Cin][k], bias DEVICE [Cout] or NULL; y DEVICE (B, Cout).
 * With r == 1 the buffer may be NULL.  Asynchronous on the context's stream. */
int pk_op_conv1d_cell_step(pk_ctx* ctx, float* buffer, const float* x_t, const float* weight, const float* bias,
                           int32_t B, int32_t Cin, int32_t Cout, int32_t k, int32_t dilation, float* y);

/* Plain row-major product y[M][N] = x[M][K] . w[K][N] (+ bias[N]) on the exact-fp32 MFMA GEMM: the
 * `paddle.matmul(self.weight, spectrogram)` of MelScale.forward (modules/audio.py:226-229) with rows =
 * (batch, frame).  x, y device; w, bias (or NULL) HOST.  Synchronous (the weight is packed per call). */
int pk_op_matmul(pk_ctx* ctx, const float* x, int32_t M, int32_t K, int32_t N, const float* w,
                 const float* bias, float* y);

/* expand (modules/expansion.py:19-37; LengthRegulator.expand length_regulator.py:46-66 without the alpha
 * scaling): token t of utterance b is repeated durations[b][t] times; sequences shorter than the longest are
 * zero-padded.  encodings (B, T, C) device; durations HOST int64 (B, T), >= 0; out (B, t_dec, C) device with
 * t_dec = max_b sum_t durations[b][t], which the caller computes to size `out` (0 is allowed: nothing is written). */
int pk_op_expand(pk_ctx* ctx, const float* encodings, const int64_t* durations, int32_t B, int32_t T, int32_t C,
                 int32_t t_dec, float* out);

/* ------------------------------------------ the engine's shared GEMMs exactly as the models launch them */
/* These three run the kernels every dense layer of every model goes through (the implicit-conv tile GEMM with its
 * split-fp16 variant and its row-maximum pass, and the few-rows GEMM of the autoregressive decoders) with every
 * feature of their internal argument blocks, so that they can be compared with a reference at their own edges.
 * Activations, residuals, row arrays and outputs are DEVICE pointers; weights, biases, cscale / cshift, the projection,
 * the LayerNorm parameters and the stop vector are HOST arrays, [K][N] row-major, packed per call (so the calls are
 * synchronous).  A field that is NULL / 0 switches its feature off. */
typedef struct pk_op_gemm_cfg {
    /* device */
    const float* A;            /* [M][lda] rows of the timeline; rows outside [0, M) that taps or tile tails read are
                                  supplied as zeros by the call (it copies A into a buffer with that margin) */
    const float* A2;           /* [M][lda2], Cin2 more input channels appended to K, or NULL */
    const float* res;          /* [M][ldr] */
    const float* a_amax;       /* [M] max|A[r, 0..Cin)| or an upper bound of it, or NULL: computed by the launcher */
    const float* a2_amax;      /* [M] likewise for A2 */
    const int32_t* rowvalid;   /* [M], < 0: gap row */
    const int32_t* out_rowmap; /* [M], < 0: row not stored */
    float* C;                  /* [rows][ldc]; N columns are written (N / 2 under PK gate epilogue 1) */
    float* C2;                 /* [M][ldc2]: columns >= nsplit */
    /* host */
    const float* W;            /* [wtaps * Cin + Cin2][N]; gate epilogues: columns [content (N/2) | gate (N/2)] */
    const float* bias;         /* [N] (same column order as W) */
    const float* cscale;       /* [N] */
    const float* cshift;       /* [N] */
    const float* W2;           /* epilogue 2: the [64][128] projection */
    const float* bias2;        /* [128] */
    int64_t tap_off[12];       /* ntaps > 0: tap t reads A + tap_off[t] (floats) + r * lda ... */
    int32_t tap_w[12];         /* ... against the weight rows of packed tap tap_w[t] */
    int32_t M, N, Cin;
    int32_t taps, pad;         /* ntaps == 0: tap t reads row r + t - pad (wtaps = taps) */
    int32_t ntaps, wtaps;      /* ntaps > 0: the explicit form above; wtaps = taps held by W */
    int32_t Cin2, w2_slab0;    /* w2_slab0 = first weight row of the A2 block / 16 (even) */
    int32_t lda, lda2, ldr, ldc, ldc2;
    int32_t math;              /* 0 exact fp32, 1 split fp16 (falls back to fp32 below K = 128) */
    int32_t tile;              /* split fp16: 0 = the launcher's rule, 64, 128 rows per workgroup */
    int32_t act;               /* 0 none, 1 ReLU, 2 tanh */
    int32_t epi;               /* 0 standard, 1 gate: tanh(content) * sigmoid(gate), 2 gate + projection (N == 128) */
    int32_t res_pos;           /* 0 after the activation, 1 after the affine, 2 before the activation */
    int32_t nsplit, acc2;
    int32_t kernel;            /* OUT: 0 = k_gemm (fp32), 1 = k_gemm_h3 with 64-row tiles, 2 = with 128-row tiles */
} pk_op_gemm_cfg;
/* cfg is not const: the call writes cfg->kernel. */
int pk_op_gemm(pk_ctx* ctx, pk_op_gemm_cfg* cfg);

typedef struct pk_op_rowgemm_cfg {
    /* device */
    const float* x;            /* [M][ldx] */
    const float* res;          /* [M][ldr] */
    float* y;                  /* [M][ldy] */
    float* lstm_c;             /* [M][lstm_H], updated in place; switches the LSTM-cell epilogue on */
    float* lstm_h1;            /* [M][lstm_ld1] */
    float* lstm_h2;            /* [M][lstm_ld2] */
    const uint64_t* drop_seeds;   /* [M] */
    const int32_t* stop_minlen;   /* [M] */
    const int32_t* stop_maxlen;   /* [M] */
    float* stop_probs;
    int32_t* stop_len;         /* [M] */
    int32_t* stop_ndone;       /* [1] */
    /* host */
    const float* W;            /* [K][N]; LSTM: columns [i (H) | f (H) | g (H) | o (H)] */
    const float* bias;         /* [N] */
    const float* ln_g;         /* [K] LayerNorm weight / bias of the prologue */
    const float* ln_b;
    const float* stop_w;       /* [K]: switches the stop-token head on */
    uint64_t drop_base;
    int32_t M, K, N, ldx, ldr, ldy;
    int32_t act;               /* 0 none, 1 ReLU */
    float ln_eps;
    int32_t lstm_H, lstm_ld1, lstm_ld2;
    int32_t dropout, drop_J, drop_j;
    uint32_t drop_thr;         /* keep <=> word >= drop_thr */
    float drop_scale;
    float stop_bias, stop_thr;
    int32_t stop_kind, stop_max_steps, stop_step;
} pk_op_rowgemm_cfg;
int pk_op_rowgemm(pk_ctx* ctx, const pk_op_rowgemm_cfg* cfg);

/* amax[r] = max|A[r, 0..C)| for r0 <= r < r1 (device pointers; rows r0..r1-1 of both must exist, r0 may be negative).
 * Asynchronous on the context's stream. */
int pk_op_row_amax(pk_ctx* ctx, const float* A, int64_t lda, int32_t C, int64_t r0, int64_t r1, float* amax);

#ifdef __cplusplus
}
#endif
#endif /* PK_SYNTH_H */
