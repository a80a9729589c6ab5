/*
 * rs_asr.h — C ABI of librs_asr.so, the MI355X (gfx950) FastConformer-RNNT inference path.
 *
 * The reference (reazon-research/ReazonSpeech) has NO FFI / plugin boundary for this path:
 * its only interface is the Python pair load_model()/transcribe()
 * (pkg/nemo-asr/src/transcribe.py:9-28, :30-60) which hands everything to NeMo at two call
 * sites (EncDecRNNTBPEModel.from_pretrained :26-28, model.transcribe :48-53).  This header is
 * the boundary introduced *underneath* that pair: each entry point below names
 * the reference-side step it replaces.  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / C++ types.
 *   - The CALLER owns every device buffer (weights, activations, workspace); the library never
 *     allocates or frees device memory.  All pointers are device pointers unless named host_*.
 *   - Every function returns RS_OK (0) or a negative RS_E* code; rs_last_error() returns a
 *     message for the last failure on that context (thread-compatible, not re-entrant: one
 *     context per stream).  No exit/abort, no C++ exception crosses the ABI.
 *   - Work is enqueued asynchronously on the given hipStream_t (passed as void*; NULL = the
 *     default stream).  Nothing synchronises unless stated.
 *   - bf16 tensors are raw uint16 bit patterns (round-to-nearest-even of the f32 value).
 */
#ifndef RS_ASR_H
#define RS_ASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 7

enum {
    RS_OK = 0,
    RS_EINVAL = -1,      /* bad argument / shape */
    RS_EMISSING = -2,    /* a required weight tensor was not registered */
    RS_EWORKSPACE = -3,  /* workspace too small */
    RS_EHIP = -4,        /* a HIP runtime call failed */
    RS_EOVERFLOW = -5,   /* decode output buffer (u_max) too small for some utterance */
    RS_ESTATE = -6       /* call order violated (e.g. forward before rs_finalize) */
};

typedef struct rs_ctx rs_ctx;

/* Model dimensions: what NeMo reads from model_config.yaml inside the .nemo checkpoint
 * (reference: pkg/nemo-asr/src/transcribe.py:26-28 [UPSTREAM]). */
typedef struct rs_dims {
    int32_t n_mels;        /* 80 */
    int32_t n_fft;         /* 512 (only 512 is built) */
    int32_t win_length;    /* 400 */
    int32_t hop_length;    /* 160 */
    float preemph;         /* 0.97, 0 disables */
    float log_guard;       /* 2^-24 */
    float norm_eps;        /* 1e-5, added to the per-feature std */
    int32_t d_model;       /* 1024 */
    int32_t n_heads;       /* 8 (head_dim must be 128) */
    int32_t ff_dim;        /* 4096 */
    int32_t n_layers;      /* 24 */
    int32_t conv_kernel;   /* 9 */
    int32_t sub_channels;  /* 256 */
    int32_t sub_stages;    /* 3 (x8) */
    int32_t xscaling;      /* 1: multiply the subsampling output by sqrt(d_model) */
    float ln_eps;          /* 1e-5 */
    int32_t att_left;      /* -1 = unlimited */
    int32_t att_right;     /* -1 = unlimited */
    int32_t n_global;      /* global tokens of the local-attention variant (0 = none) */
    int32_t n_logits;      /* vocab + 1 (3001) */
    int32_t blank_id;      /* 3000 */
    int32_t pred_hidden;   /* 640 */
    int32_t pred_layers;   /* 2 */
    int32_t joint_hidden;  /* 640 */
    int32_t max_symbols;   /* 10 */
    /* ---- model family switches (ABI 3).  All zero = NeMo FastConformer-RNNT, the path everything above describes.  The
     * ESPnet2 Conformer-Transducer of reazonspeech.espnet.asr (pkg/espnet-asr/src/transcribe.py:26-32) sets all five. ---- */
    int32_t frontend_kind; /* 0: NeMo AudioToMelSpectrogramPreprocessor.  1: ESPnet DefaultFrontend + GlobalMVN — reflect edge
                              padding, 1 + L / hop frames, log(max(x, log_guard)), (x - "fe.mvn_mean") * "fe.mvn_istd"; preemph
                              must be 0 */
    int32_t sub_kind;      /* 0: dw_striding x 2^sub_stages.  1: ESPnet Conv2dSubsampling x4 — Conv2d(1, C, 3, 2) ReLU
                              Conv2d(C, C, 3, 2) ReLU without padding ("sub.conv0.*" f32 tap-major, "sub.conv1.w" bf16 [C][9C] with K
                              ordered (kernel row, kernel column, channel)), Linear(C * F2, d_model); sub_stages must be 2 */
    int32_t final_norm;    /* 1: a LayerNorm after the last block ("final_norm.g" / ".b"; ESPnet encoder.after_norm) */
    int32_t joint_act;     /* joint activation: 0 = ReLU (NeMo), 1 = tanh (ESPnet JointNetwork); tanh decodes with the exact
                              (un-screened) joint kernels */
    int32_t ctc_vocab;     /* > 0: a CTC head Linear(d_model, ctc_vocab) is registered with its rows padded to Vp = the next
                              multiple of 4 ("ctc.w" bf16 [Vp][d_model], "ctc.b" f32 [Vp]; the padding rows are never read back:
                              the softmax runs over ctc_vocab columns and writes 0 to the rest); see rs_encoder_set_ctc_out */
} rs_dims;

/* Dimensions of the Zipformer2 transducer of reazonspeech.k2.asr: what sherpa-onnx reads out of the three ONNX files the
 * reference hands it (pkg/k2-asr/src/huggingface.py:73-83; [UPSTREAM] icefall zipformer recipe: --num-encoder-layers,
 * --feedforward-dim, --num-heads, --encoder-dim, --cnn-module-kernel, --downsampling-factor, --query-head-dim, ...). */
typedef struct rs_k2_dims {
    int32_t n_mels;            /* 80 (feature_dim, huggingface.py:80) */
    int32_t frame_length;      /* 400 samples */
    int32_t frame_shift;       /* 160 samples */
    float preemph;             /* 0.97 (kaldi-native-fbank default) */
    int32_t embed_c1, embed_c2, embed_c3;   /* encoder_embed conv channels: 8, 32, 128 */
    int32_t n_stacks;          /* 6 */
    int32_t encoder_dim[8];    /* 192,256,512,768,512,256 */
    int32_t num_layers[8];     /* 2,2,4,5,4,2 */
    int32_t ff_dim[8];         /* 512,768,1536,2048,1536,768 */
    int32_t num_heads[8];      /* 4,4,4,8,4,4 */
    int32_t cnn_kernel[8];     /* 31,31,15,15,15,31 (7, 15 and 31 are built) */
    int32_t downsampling[8];   /* 1,2,4,8,4,2 */
    int32_t query_head_dim;    /* 32 */
    int32_t value_head_dim;    /* 12 */
    int32_t pos_head_dim;      /* 4 */
    int32_t pos_dim;           /* 48 (host side only: the position tables arrive projected) */
    int32_t vocab_size;        /* lines of tokens.txt */
    int32_t decoder_dim;       /* 512 */
    int32_t joiner_dim;        /* 512 */
    int32_t context_size;      /* 2 */
    int32_t blank_id;          /* 0 */
    int32_t unk_id;            /* id of "<unk>", -1 = none: sherpa-onnx's greedy search does not emit it */
} rs_k2_dims;

/* ---- context ------------------------------------------------------------------------- */

/* Replaces: model object construction inside EncDecRNNTBPEModel.from_pretrained
 * (pkg/nemo-asr/src/transcribe.py:26-28).  `device` is the HIP device ordinal. */
int rs_create(rs_ctx** out, int device, const rs_dims* dims);
/* The same for reazonspeech.k2.asr — replaces: sherpa_onnx.OfflineRecognizer.from_transducer(encoder, decoder, joiner, ...)
 * (pkg/k2-asr/src/huggingface.py:73-83).  The context answers the SAME stage entry points: rs_set_tensor / rs_finalize,
 * rs_workspace_bytes, rs_mel_frames ((n + shift / 2) / shift kaldi-style frames), rs_enc_frames (((T - 7) / 2 + 1) / 2),
 * rs_frontend_logmel (kaldi-native-fbank features: snip_edges false with reflected edges, per-frame DC removal and
 * pre-emphasis, povey window, log(max(mel energy, FLT_EPSILON)), no normalisation), rs_encoder_forward (encoder_embed +
 * Zipformer2 stacks + joiner.encoder_proj, csrc/k_zipformer.hip) and rs_rnnt_greedy (stateless decoder + tanh joiner, one
 * symbol per frame, `<unk>` treated as blank: sherpa-onnx OfflineTransducerGreedySearchDecoder).  Tensor names: DESIGN.md
 * "reazonspeech.k2.asr". */
int rs_k2_create(rs_ctx** out, int device, const rs_k2_dims* dims);
/* Parity taps of a Zipformer context (tests only): embed_out f32 [B*T3][encoder_dim[0]] (encoder_embed's output) and stack_out,
 * the stacks' outputs f32 [B*T3][encoder_dim[s]] one after the other; NULL disables. */
int rs_k2_encoder_set_taps(rs_ctx* ctx, float* embed_out, float* stack_out);

/* ---- reazonspeech.avsr: the AV-HuBERT encoder-decoder (csrc/k_avsr.hip) ---------------------------------------------------------
 * The reference is in-tree torch code: AVHubertForConditionalGeneration (pkg/avsr/src/avhubert/modeling_avhubert.py:216-391) over
 * AVHubertModel (:119-213: audio Linear, Conv3d + ResNet-18 video front-end modeling_resnet.py:140-178, concatenation, LayerNorm,
 * post_extract_proj, transformers' HubertEncoder) and AVHubertDecoder (decoder.py:467-617).  Everything is float32, as in the
 * reference.  Tensor names and layouts: reazonspeech_amd/runtime/avsr_weights.py: prepare_weights_avsr. */
typedef struct rs_avsr_dims {
    int32_t encoder_layers;        /* 12  (configuration_avhubert.py:9-13) */
    int32_t encoder_embed_dim;     /* 768 */
    int32_t encoder_ffn_dim;       /* 3072 */
    int32_t encoder_heads;         /* 12 */
    int32_t conv_pos;              /* 128: kernel of the positional convolution (even) */
    int32_t conv_pos_groups;       /* 16 */
    int32_t audio_feat_dim;        /* 104 = 4 stacked 26-dim log filterbank frames (feature_extraction_avhubert.py:120-137) */
    int32_t fuse_concat;           /* 1: modality_fuse "concat" (the only form built) */
    int32_t image_size;            /* 88 (feature_extraction_avhubert.py:24) */
    int32_t decoder_layers;        /* 6 */
    int32_t decoder_embed_dim;     /* 768 (== encoder_embed_dim) */
    int32_t decoder_ffn_dim;       /* 3072 */
    int32_t decoder_heads;         /* 4 */
    int32_t max_positions;         /* 2048 rows of the sinusoidal table */
    int32_t vocab_size;
    float layer_norm_eps;          /* 1e-5 */
} rs_avsr_dims;
/* Replaces: AVHubertForConditionalGeneration.__init__ / from_pretrained (modeling_avhubert.py:216-254).  The context takes
 * rs_set_tensor / rs_finalize / rs_destroy / rs_last_error and the rs_avsr_* stage functions below (the transducer stages do not
 * apply to it). */
int rs_avsr_create(rs_ctx** out, int device, const rs_avsr_dims* dims);
size_t rs_avsr_workspace_bytes(const rs_ctx* ctx, int B, int T);
/* Replaces: AVHubertModel.forward (modeling_avhubert.py:162-213).
 *   input_values f32[B][T][audio_feat_dim], pixel_values f32[B][T][image_size][image_size] (the reference's [B][T][1][H][W]),
 *   padding_mask f32[B][T] (nonzero = padding frame; the reference's padding_mask, :192-195) -> enc_out f32[B][T][encoder_embed_dim]
 *   = last_hidden_state.  Padded frames go through the front-ends like any other (as in the reference); their encoder inputs are
 *   zeroed and they are masked as attention keys. */
int rs_avsr_encoder_forward(rs_ctx* ctx, const float* input_values, const float* pixel_values, const float* padding_mask, int B,
                            int T, float* enc_out, void* workspace, size_t workspace_bytes, void* stream);
/* Parity taps (tests only; NULL disables): video = feature_extractor_video output f32[B*T][d], fused_ln = avhubert.layer_norm output
 * f32[B*T][2d], enc_ln = encoder.layer_norm output f32[B*T][d], layer_out = the listed encoder layers' outputs one after the other. */
int rs_avsr_encoder_set_taps(rs_ctx* ctx, float* video, float* fused_ln, float* enc_ln, float* layer_out, const int32_t* layer_ids,
                             int n_layer_ids);
/* Replaces: the decoder half of AVHubertForConditionalGeneration.forward inside generate() (modeling_avhubert.py:283-298,
 * decoder.py:488-617), one token per call with a KV cache (the reference re-feeds the prefix and re-runs the encoder every step,
 * :372-391; same results).  rows = B * beams hypothesis rows, row = clip * beams + beam (transformers' flattening).
 *   rs_avsr_decoder_begin   cross-attention keys / values of every layer from enc f32[B][T][d]; call once per batch
 *   rs_avsr_decoder_step    tokens i32[rows] = the token at position `step` of every row (step 0: the bos prompt); src_rows i32[rows]
 *                           or NULL = the row whose prefix each row continues (beam search re-parenting; give it at EVERY step >= 1
 *                           or at none); padding_mask as above; -> logits f32[rows][vocab_size rounded up to 4] of position `step`
 * `state` is caller-owned device memory of rs_avsr_decoder_state_bytes(B, T, beams, max_len) bytes, untouched between calls. */
size_t rs_avsr_decoder_state_bytes(const rs_ctx* ctx, int B, int T, int beams, int max_len);
int rs_avsr_decoder_begin(rs_ctx* ctx, const float* enc, int B, int T, int beams, int max_len, void* state, size_t state_bytes,
                          void* stream);
int rs_avsr_decoder_step(rs_ctx* ctx, const int32_t* tokens, const int32_t* src_rows, int step, const float* padding_mask, int B,
                         int T, int beams, int max_len, float* logits, void* state, size_t state_bytes, void* stream);

/* ---- reazonspeech.avsr: generate()'s searches on the device (csrc/k_avsr_search.hip; added within ABI 7) ---------------------------
 * Replaces: what transformers' GenerationMixin does with the logits inside AVHubertForConditionalGeneration.generate()
 * (modeling_avhubert.py:216,372-391; README.rst:41 `model.generate(**inputs, num_beams=5, max_new_tokens=256)`):
 *   greedy != 0   GenerationMixin._sample with do_sample False: argmax per row over v < vocab, EQUAL VALUES TAKE THE LOWER INDEX; a
 *                 row that emitted eos is fed / filled with pad_token_id; stops when no row is unfinished.  beams must be 1.
 *   greedy == 0   GenerationMixin._beam_search (v4.50+, early_stopping False, one eos token) with `beams` = num_beams in 1..8: per clip
 *                 and step the 2 beams best (beam, token) continuations by log_softmax + running score, ORDERED BY VALUE DESCENDING,
 *                 THEN FLAT INDEX beam * vocab + token ASCENDING; the `beams` best that do not end run on (equal values: the earlier
 *                 candidate); those among the first `beams` that end (eos, or the last position) compete with score / (generated
 *                 length) ** length_penalty for the clip's finished slots (equal scores: the earlier position, finished slots before
 *                 candidates); a clip stops adding finished hypotheses once its best running score cannot beat its worst finished
 *                 one; the search ends when no clip can improve or nothing can continue.
 * Arithmetic is float32 in the order of reazonspeech_amd/avsr/generation.py.  log_softmax of a row x: m = max x; S = sum of
 * rs_expf(x[v] - m) with thread t of 256 adding its columns v = t, t + 256, ... in increasing v and the 256 partial sums combined by a
 * binary tree (stride 128, 64, ..., 1: p[t] += p[t + stride]); logp[v] = ((x[v] - m) - rs_logf(S)) + running score.  The length
 * divisor is (float)pow((double)position, (double)length_penalty) computed on the host. */
typedef struct rs_avsr_search {
    int32_t beams;                 /* hypothesis rows per clip, 1..8 */
    int32_t max_new_tokens;        /* >= 1; 1 + max_new_tokens <= max_positions */
    int32_t bos_token_id;          /* the decoder prompt is this one token */
    int32_t eos_token_id;
    int32_t pad_token_id;
    int32_t greedy;                /* != 0: _sample (beams must be 1); 0: _beam_search (also with beams 1) */
    float length_penalty;          /* beam search only; transformers' default 1.0 */
} rs_avsr_search;
/* The search alone, step by step over caller-supplied logits f32[B * beams][vocab rounded up to 4] (columns >= vocab are never
 * read) — this family's single-operator hook; rs_avsr_generate is built from it.  `state` is caller-owned device memory of
 * rs_avsr_search_state_bytes(B, beams, 1 + max_new_tokens) bytes.  Call _begin, then _step for step = 0, 1, ... in order; nothing
 * synchronises except _peek and _finish.  A step issued after the search has stopped changes nothing.
 *   rs_avsr_search_rows     device pointers (inside `state`) to tokens i32[rows] and src_rows i32[rows]: what the next
 *                           rs_avsr_decoder_step takes (greedy: pass src_rows NULL to the decoder)
 *   rs_avsr_search_peek     host copies (any may be NULL) of tokens, src_rows, running scores f32[rows], finished scores f32[rows], and
 *                           *goes_on = 1 if step `step` is to run (the device's go word of that step: greedy, the number of unfinished
 *                           rows; beam, low half = clips that can improve, high half = clips with a candidate that does not end)
 *   rs_avsr_search_finish   sequences i32[B][1 + max_new_tokens] (bos first, pad_token_id past a clip's end), lengths i32[B], scores
 *                           f32[B] (beam: the best finished hypothesis and its score; NULL allowed; greedy: zeros); device pointers
 * RS_EINVAL for a context that is not avsr, beams outside 1..8, 1 + max_new_tokens > max_positions, vocab < 4; RS_EWORKSPACE for a
 * short state.  The *_state_bytes queries return 0 for such arguments. */
size_t rs_avsr_search_state_bytes(const rs_ctx* ctx, int B, int beams, int max_len);
int rs_avsr_search_begin(rs_ctx* ctx, const rs_avsr_search* search, int B, int vocab, void* state, size_t state_bytes, void* stream);
int rs_avsr_search_step(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, int B, int vocab, void* state,
                        size_t state_bytes, void* stream);
int rs_avsr_search_rows(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, const int32_t** tokens,
                        const int32_t** src_rows);
int rs_avsr_search_peek(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int step, int32_t* tokens,
                        int32_t* src_rows, float* run_scores, float* fin_scores, int32_t* goes_on, void* stream);
int rs_avsr_search_finish(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int32_t* sequences,
                          int32_t* lengths, float* scores, void* stream);
/* Replaces: generate() after the encoder.  enc f32[B][T][d] and padding_mask f32[B][T] as for rs_avsr_decoder_*; runs
 * rs_avsr_decoder_begin once, then per token rs_avsr_decoder_step on the tokens / src_rows the last selection left on the device and
 * rs_avsr_search_step on its logits.  The host reads one 4-byte go word per step, two steps behind the launches; no other host
 * traffic per token.  Outputs as rs_avsr_search_finish.  `state`: rs_avsr_generate_state_bytes(B, T, beams, 1 + max_new_tokens)
 * bytes (decoder state + search state + logits).  Synchronises the stream internally (the trip count depends on the data). */
size_t rs_avsr_generate_state_bytes(const rs_ctx* ctx, int B, int T, int beams, int max_len);
int rs_avsr_generate(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search,
                     int32_t* sequences, int32_t* lengths, float* scores, void* state, size_t state_bytes, void* stream);
/* The same searches with transformers' logits processors and beam-search switches (still ABI 7; the entry points above are these
 * with neutral options and stay bit-identical).  Semantics are those of transformers.generation (logits_process.py; utils.py
 * _get_logits_processor, _sample, _beam_search): per hypothesis row, over its own prefix with bos,
 *   1. repetition_penalty p: s = s < 0 ? s * p : s / p for every token of the prefix (one float32 operation)
 *   2. no_repeat_ngram_size n: -inf for a token that would complete an n-gram already in the prefix (n = 1: every token seen; nothing
 *      while the prefix has fewer than n tokens)
 *   3. min_new_tokens m: -inf for eos while fewer than m tokens have been generated
 * applied, greedy, to the raw logits before the argmax, and, beam, to (x[v] - m) - rs_logf(S) before the running score is added, with
 * m and S those of the raw logits (no renormalisation).  -inf candidates follow the same order (value, then flat index).
 *   early_stopping 0  transformers' False: as above
 *                  1  True: a clip whose `beams` finished slots are full takes no more, and the search ends when every clip is full
 *                  2  "never": with length_penalty > 0 the can-improve test divides the best running score by
 *                     (float)pow((double)max_new_tokens, (double)length_penalty) instead of by the current length's divisor
 *   num_return_sequences n in 1..beams: _finish / _generate write the n best finished hypotheses of every clip, clip-major:
 *      sequences i32[B * n][1 + max_new_tokens], lengths i32[B * n] (0: the slot never finished and holds bos + pad), scores f32[B * n]
 * RS_EINVAL for repetition_penalty <= 0, a negative size, early_stopping outside 0..2, n outside 1..beams, greedy with n > 1. */
typedef struct rs_avsr_search_opts {
    float repetition_penalty;      /* > 0; 1.0: none */
    int32_t no_repeat_ngram_size;  /* >= 0; 0: none */
    int32_t min_new_tokens;        /* >= 0 */
    int32_t early_stopping;        /* 0 False, 1 True, 2 "never" (beam search only) */
    int32_t num_return_sequences;  /* 1..beams (greedy: 1) */
} rs_avsr_search_opts;
/* `opts` NULL means neutral.  The state of the _opts forms is rs_avsr_search_state_bytes_opts / rs_avsr_generate_state_bytes_opts
 * bytes (vocab: large vocabularies keep their per-row token marks there); its front has the layout of the plain forms, so
 * rs_avsr_search_rows serves both.  rs_avsr_search_peek_opts is _peek whose *goes_on also honours early_stopping 1. */
size_t rs_avsr_search_state_bytes_opts(const rs_ctx* ctx, int B, int beams, int max_len, int vocab, const rs_avsr_search_opts* opts);
int rs_avsr_search_begin_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, int vocab, void* state,
                              size_t state_bytes, void* stream);
int rs_avsr_search_step_opts(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, const rs_avsr_search_opts* opts,
                             int B, int vocab, void* state, size_t state_bytes, void* stream);
int rs_avsr_search_peek_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state,
                             size_t state_bytes, int step, int32_t* tokens, int32_t* src_rows, float* run_scores, float* fin_scores,
                             int32_t* goes_on, void* stream);
int rs_avsr_search_finish_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state,
                               size_t state_bytes, int32_t* sequences, int32_t* lengths, float* scores, void* stream);
size_t rs_avsr_generate_state_bytes_opts(const rs_ctx* ctx, int B, int T, int beams, int max_len, const rs_avsr_search_opts* opts);
int rs_avsr_generate_opts(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search,
                          const rs_avsr_search_opts* opts, int32_t* sequences, int32_t* lengths, float* scores, void* state,
                          size_t state_bytes, void* stream);
/* The same searches, recording what they otherwise discard after each step (still ABI 7; the _opts forms are these without the
 * recording and stay bit-identical; nothing the search decides changes).  Replaces: transformers.generation's
 * `output_scores=True` / `return_dict_in_generate=True` bookkeeping in utils.py — `scores += (next_token_scores,)` of _sample,
 * `all_scores += (log_probs,)` and the `running_beam_indices` / `beam_indices` gathers of _beam_search — and
 * GenerationMixin.compute_transition_scores (the gather of scores[p][beam_indices[., p]][sequences[., p + 1]], and its log_softmax for
 * normalize_logits=True).  Per returned hypothesis and generated position p (sequence index p + 1):
 *   token_scores  f32[B * n][max_new_tokens]  the processed score of the token chosen there, transformers' scores[p][row][token]:
 *                 greedy, the logit after the processors above; beam, (x[v] - m) - rs_logf(S) after them, before the running score
 *   token_lse     f32[B * n][max_new_tokens]  the log-sum-exp of that row's processed scores over v < vocab at that step: M = max, Z =
 *                 sum of rs_expf(s[v] - M) in the order of S above (thread t adds columns t, t + 256, ... in increasing v, then the
 *                 binary tree of stride 128 .. 1; a -inf column adds exactly 0.0f), lse = M + rs_logf(Z); token_scores - token_lse is
 *                 the token's log-probability under the processed distribution (normalize_logits=True)
 *   beam_indices  i32[B * n][max_new_tokens]  beam search: the flat row clip * beams + beam whose scores the token was taken from (that
 *                 step's src_rows; transformers' beam_indices); greedy: all -1, NULL allowed
 * clip-major like `sequences`; with g = lengths - 1 generated tokens (eos included), positions p >= g hold 0.0f, 0.0f and -1, as does a
 * slot that never finished.  steps_run i32[1] (NULL allowed): the number of steps the search ran.  All device pointers.
 *   step_scores   f32[max_new_tokens][B * beams][vocab rounded up to 4] or NULL, on _step_scored and _generate_scored: step `step`
 *                 writes the whole processed row of every hypothesis row, in the order it read them (transformers' `scores`
 *                 tuple): columns v < vocab the processed score (-inf where banned), the padding columns 0.  Only steps that ran write.
 * The state is rs_avsr_search_state_bytes_scored / rs_avsr_generate_state_bytes_scored bytes (the histories live in it, re-parented
 * with the prefixes); its front has the plain layout, so rs_avsr_search_rows serves it.  A state begun with _begin_scored is
 * stepped, peeked and finished with the _scored forms only.  RS_EINVAL, before anything is enqueued, for a context that is not
 * avsr, a null token_scores / token_lse, or a null beam_indices in beam search; RS_EWORKSPACE for a short state; the
 * *_state_bytes_scored queries return 0 for invalid arguments. */
size_t rs_avsr_search_state_bytes_scored(const rs_ctx* ctx, int B, int beams, int max_len, int vocab, const rs_avsr_search_opts* opts);
int rs_avsr_search_begin_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, int vocab, void* state,
                                size_t state_bytes, void* stream);
int rs_avsr_search_step_scored(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, const rs_avsr_search_opts* opts,
                               float* step_scores, int B, int vocab, void* state, size_t state_bytes, void* stream);
int rs_avsr_search_peek_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state,
                               size_t state_bytes, int step, int32_t* tokens, int32_t* src_rows, float* run_scores, float* fin_scores,
                               int32_t* goes_on, void* stream);
int rs_avsr_search_finish_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state,
                                 size_t state_bytes, int32_t* sequences, int32_t* lengths, float* scores, float* token_scores,
                                 float* token_lse, int32_t* beam_indices, int32_t* steps_run, void* stream);
size_t rs_avsr_generate_state_bytes_scored(const rs_ctx* ctx, int B, int T, int beams, int max_len, const rs_avsr_search_opts* opts);
int rs_avsr_generate_scored(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search,
                            const rs_avsr_search_opts* opts, float* step_scores, int32_t* sequences, int32_t* lengths, float* scores,
                            float* token_scores, float* token_lse, int32_t* beam_indices, int32_t* steps_run, void* state,
                            size_t state_bytes, void* stream);
void rs_destroy(rs_ctx* ctx);
const char* rs_last_error(const rs_ctx* ctx);
int rs_abi_version(void);

/* Register one prepared weight tensor by name (device pointer, caller-owned, must outlive the
 * context).  Names and layouts: DESIGN.md §"Weights in HBM".  Replaces: load_state_dict inside
 * from_pretrained (transcribe.py:26-28).
 * Optional derived tensors "L{i}.att.pos_proj" (bf16, same shape as "pos.table"): the position
 * table already multiplied by layer i's linear_pos weight (one rs_gemm_bf16 call per layer at load
 * time); when registered, rs_encoder_forward skips that projection in every call.
 * "L{i}.conv.pw1.w" / ".b" (the conv module's first pointwise convolution, 2*d_model output rows) are registered
 * with their rows interleaved in blocks of 32: rows 64j .. 64j+31 are the value rows 32j .. 32j+31 of NeMo's
 * pointwise_conv1, rows 64j+32 .. 64j+63 the matching gate rows d_model + 32j ..: a GLU pair then sits in one
 * MFMA lane of the GEMM and is applied in its epilogue (RS_GEMM_GLU). */
int rs_set_tensor(rs_ctx* ctx, const char* name, const void* dev_ptr, size_t nbytes);
/* Check that every tensor the dims require is present; must precede any forward call. */
int rs_finalize(rs_ctx* ctx);

/* Bytes of scratch the three stage functions need for a batch of B utterances whose padded
 * sample count is at most max_samples (pad included). */
size_t rs_workspace_bytes(const rs_ctx* ctx, int B, int max_samples);

/* Shape helpers (host arithmetic, no device work).  Like every query that returns a size or a frame count, they answer 0 for
 * a null context and for a context of a family they are not defined for (an AV-HuBERT context), and write no error text:
 * their context is const. */
int rs_mel_frames(const rs_ctx* ctx, int n_samples);   /* floor(L / hop) */
int rs_enc_frames(const rs_ctx* ctx, int n_mel_frames); /* three k3 s2 p1 convs */

/* ---- host staging (A4: `torch.from_numpy` + list wrap, transcribe.py:46-50, for a whole batch) -------------------
 * Pure host function, no device work: gathers `n_rows` utterances (host float32, 16 kHz mono, un-padded) into the
 * caller's pinned staging matrix dst[total_rows][dst_pitch], zero-filling every row from its length up to `width`
 * (the batch's padded extent) and writing the lengths (0 for rows n_rows .. total_rows - 1: a short last batch).
 * One call per batch instead of one interpreter-level copy per utterance: a Python binding releases its interpreter lock
 * for the call, so the staging of batch i+2 does not contend with host post-processing of batch i. */
int rs_host_stage_rows(float* dst, size_t dst_pitch, int width, const float* const* rows, const int32_t* lens,
                       int n_rows, int total_rows, int32_t* dst_lens);

/* ---- stage 1: log-mel front-end -------------------------------------------------------
 * Replaces: pad_audio (pkg/nemo-asr/src/audio.py:70-83, folded into the load: the kernel
 * reads `audio[b][i - pad_left]` and treats everything outside [0, lens[b]) as 0) and NeMo's
 * AudioToMelSpectrogramPreprocessor reached through model.transcribe (transcribe.py:48-53):
 * pre-emphasis, STFT(512, hann 400, hop 160, centre, zero pad), power, Slaney mel 80,
 * log(x + 2^-24), per-feature normalisation over the valid frames, zeroed padding.
 *
 *   audio   f32[B][audio_stride]   raw (un-padded) samples
 *   lens    i32[B]                  valid samples per utterance (un-padded)
 *   feats   f32[B][t_max][n_mels]   t_max = rs_mel_frames(max(lens) + pad_left + pad_right)
 *   n_frames i32[B]                 valid frames per utterance (written)
 */
int rs_frontend_logmel(rs_ctx* ctx, const float* audio, const int32_t* lens, int B,
                       int audio_stride, int pad_left, int pad_right, int t_max,
                       float* feats, int32_t* n_frames, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- stage 2: FastConformer encoder + joint encoder projection --------------------------
 * Replaces: ConformerEncoder.forward and RNNTJoint.enc inside model.transcribe
 * (transcribe.py:48-53): dw-striding x8 subsampling, 24 x [1/2 FFN, rel-pos MHSA, conv
 * module, 1/2 FFN, LayerNorm], Linear d_model -> joint_hidden.
 *
 *   feats, n_frames      as produced by rs_frontend_logmel
 *   enc_out  f32[B][tp_max][d_model]      (may be NULL if not wanted) tp_max = rs_enc_frames(t_max)
 *   joint_enc f32[B][tp_max][joint_hidden]
 *   enc_lens i32[B]
 */
int rs_encoder_forward(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max,
                       float* enc_out, float* joint_enc, int32_t* enc_lens,
                       void* workspace, size_t workspace_bytes, void* stream);

/* A HIP stream restricted to a set of compute units (bit i of cu_mask = CU i may run this stream's workgroups;
 * hipExtStreamCreateWithCUMask), or, with cu_mask == NULL, a plain non-blocking stream of the given priority.
 * The two-stage pipeline can confine the latency-bound decode loop to a slice of the chip so that its many small
 * launches stop delaying the encoder GEMMs' tile rounds on the other CUs.  No reference counterpart. */
int rs_stream_create(void** stream_out, int device, const uint32_t* cu_mask, int n_words, int priority);
int rs_stream_destroy(void* stream);

/* Scheduling options of a context (no reference counterpart).
 *   "fuse_glu"           1 (default): the conv module's GLU is applied to the float32 accumulators of the pw1 GEMM in its
 *                        epilogue, for EVERY batch size (one rounding point: an utterance's arithmetic does not depend on
 *                        the batch it rides in); 0 = the plain pw1 product is stored and the depthwise kernel applies the
 *                        GLU (moves one bf16 rounding; A/B and layout tests; $RS_FUSE_GLU).
 *   "defer_out_norm"     1 (default): the float32 rows of a layer's output LayerNorm are not stored — their one reader, the
 *                        residual operand of the next layer's first FFN, normalises the un-normed rows in its GEMM epilogue
 *                        from per-row (mean, rstd); layers with a parity tap, and the last layer, store them.  0 = every
 *                        output norm stores its rows.  Bit-identical results either way ($RS_DEFER_OUT_NORM).
 *   "decode_screen"      1 (default when the tensors joint.out.w16 / .wrm / .bpad / .wmax are registered): the joint's
 *                        output layer runs as a bf16 screening GEMM followed by an exact float32 evaluation of every
 *                        column that can still be the argmax (bit-identical result); 0 = every column in exact float32.
 *   "decode_narrow"      1 (default): LSTM / prediction-projection kernels with one 16-column tile per workgroup (4x the
 *                        workgroups, a quarter of the per-launch latency on an idle chip); 0 = the wide-tile kernels, which
 *                        need fewer free CUs per launch and do better next to the encoder GEMMs of the two-stage pipeline.
 *   "precision_f32"      0 (default): the throughput mode — bf16 GEMM operands and stored activations, float32 accumulation,
 *                        float32 residual stream.  1: the PARITY mode — rs_encoder_forward runs with float32 weights,
 *                        activations and arithmetic end to end (exact-f32 matrix-core GEMMs, IEEE exp / divide), which is what
 *                        the reference computes (pkg/nemo-asr/src/transcribe.py:26-28, :48-53: float32, no autocast).  Needs the
 *                        "<name>.f32" tensors: float32 copies of every bf16 GEMM weight (same layout; "L{i}.conv.pw1.w.f32" /
 *                        ".b.f32" in NeMo's own row order, values then gates) and "pos.table.f32"; rs_workspace_bytes
 *                        accounts for the mode once they are registered.  ~20x slower; front-end and decode are float32 in
 *                        both modes.
 *   "precision_i8"       (Zipformer contexts; default 0) 1: the INT8 mode — what onnxruntime computes from the reference's
 *                        "int8" / "int8-fp32" ONNX files (quantize_dynamic: every MatMul with a constant weight becomes
 *                        DynamicQuantizeLinear + MatMulInteger + scale Mul): rs_encoder_forward runs the "precision_f32" encoder,
 *                        and every Linear with a registered "<name>.i8" (int8 [N][K padded to 32] in the layout of "<name>.f32",
 *                        "<name>.i8.cs" int32 [N] column sums, "<name>.i8.q" f32 [4] = (sw, zw, 0, 0)) runs as rs_gemm_i8q with
 *                        (sx, zx) taken per utterance over its own rows; a quantized linear_pos ("S{s}.L{j}.attw.pos.w.i8") also
 *                        needs "pos.enc" (the relative-position encoding, f32 [2 cap - 1][pos_dim]).  Needs the "*.f32" tensors
 *                        for everything else.  Not bit-exact against onnxruntime (which has never run here): a restatement
 *                        of its int8 graph (tests/k2_int8_ref.py).
 *   "gemm_f32_x3"        (default 0) 1: the float32 products of rs_gemm_f32-class launches (the "precision_f32" encoder, the AV-HuBERT
 *                        encoder) are formed from three bf16 matrix-core terms — hi / lo split of both operands, hi.hi + hi.lo + lo.hi,
 *                        float32 accumulation: 16 mantissa bits per operand — instead of the exact v_mfma_f32_16x16x4_f32 chain:
 *                        ~2x faster.  NOT an IEEE float32 chain: a mode of its own (Python: precision="fp32x3", products="x3"),
 *                        held to the same goldens as the exact mode (tests/test_gpu_*fp32*.py, tests/test_gpu_avsr.py).
 *   "k2_cnx_fused", "k2_conv2_fused"   (Zipformer contexts; default 1) the encoder_embed's ConvNeXt pointwise pair as one kernel /
 *                        its 32 -> 128 convolution with the patches gathered into LDS; 0 = the GEMM launches they replace.  Both
 *                        forms give the same bits (tests/test_gpu_k2.py): the switch exists for that comparison. */
int rs_set_option(rs_ctx* ctx, const char* key, int value);

/* Parity taps (tests only; no reference counterpart — NeMo exposes intermediate activations through
 * forward hooks): when set, the next rs_encoder_forward calls also copy the f32 residual stream
 * [B*tp_max][d_model] after the subsampling block (sub_out) and after each listed
 * conformer layer (layer_out[k] for layer_ids[k]; rows L1-L7).  NULL / 0 disables.  layer_ids is a host array. */
int rs_encoder_set_taps(rs_ctx* ctx, float* sub_out, float* layer_out, const int32_t* layer_ids,
                        int n_layer_ids);

/* CTC posteriors (ESPnet family; replaces model.asr_model.ctc.softmax(model.asr_model.encode(...)), pkg/espnet-asr/src/ctc.py:12-27):
 * when set, the next rs_encoder_forward calls also write softmax(ctc_lo(encoder output)) — probabilities, not logarithms, as the
 * reference's blank finder (ctc.py:29-58) and its ctc_segmentation call (ctc.py:60-75) consume them — to probs f32
 * [B*tp_max][Vp] (Vp = ctc_vocab rounded up to a multiple of 4: the row pitch; columns >= ctc_vocab are 0) and / or only the
 * blank column to blank_prob f32 [B*tp_max].  Either may be NULL; both NULL disables. */
int rs_encoder_set_ctc_out(rs_ctx* ctx, float* probs, float* blank_prob);

/* ---- stage 3: RNN-T greedy decode -------------------------------------------------------
 * Replaces: decoding.rnnt_decoder_predictions_tensor inside model.transcribe
 * (transcribe.py:48-53) — prediction network (Embedding + LSTM), joint (ReLU + Linear),
 * argmax, max_symbols loop — in its batched-greedy form (the north-star's decode strategy;
 * the reference post-processing expects ALSD-shaped output, see Hypothesis.from_greedy).
 *
 *   joint_enc f32[B][tp_max][joint_hidden], enc_lens i32[B]
 *   ids     i32[B][u_max]   emitted token ids
 *   frames  i32[B][u_max]   encoder frame index each token was emitted at
 *   n_ids   i32[B]
 * Synchronises the stream internally (the trip count is data dependent).  Returns
 * RS_EOVERFLOW if an utterance would emit more than u_max tokens.
 */
int rs_rnnt_greedy(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max,
                   int u_max, int32_t* ids, int32_t* frames, int32_t* n_ids,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- stage 3b: RNN-T alignment-length synchronous beam search (ALSD) ----------------------
 * Replaces: the same call as rs_rnnt_greedy (transcribe.py:48-53) when the checkpoint's decoding
 * strategy is "alsd" — what the reference's post-processing was written for (decode.py:29,38-41:
 * "NeMo prepends a blank token to y_sequence with ALSD"; decode.py:48 converts alignment steps to
 * frames).  [UPSTREAM] BeamRNNTInfer.align_length_sync_decoding; the evaluation order of every float
 * is documented in oracle/rnnt_alsd.c and the results are bit-identical to it.
 *
 *   beam              hypotheses kept per utterance (1..8)
 *   max_target_ratio / max_target_abs
 *                     label budget per utterance: max_target_abs when >= 0, else
 *                     (int)(max_target_ratio * enc_lens[b]); the search runs enc_lens[b] + budget steps
 *   flags             RS_ALSD_SCORE_NORM: rank finished hypotheses by score / (labels + 1)
 *                     RS_ALSD_MERGE: drop recombined duplicates from the beam (default keeps them)
 *   ids    i32[B][out_cap]  labels of the best hypothesis (no leading blank)
 *   steps  i32[B][out_cap]  alignment index i = frame + labels-before of each label
 *   n_ids  i32[B],  scores f32[B] (log-probability of the best hypothesis)
 * The workspace is separate from rs_workspace_bytes (it grows with beam and the alignment length):
 * rs_rnnt_alsd_workspace_bytes(ctx, B, beam, tp_max, max_target_ratio, max_target_abs).
 * Synchronises the stream internally.  RS_EOVERFLOW if a result has more than out_cap labels. */
enum { RS_ALSD_SCORE_NORM = 1, RS_ALSD_MERGE = 2 };
size_t rs_rnnt_alsd_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio,
                                    int max_target_abs);
int rs_rnnt_alsd(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                 double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids,
                 int32_t* steps, int32_t* n_ids, float* scores, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ---- the "default" transducer beam search ---------------------------------------------------------
 * replaces: espnet2 BeamSearchTransducer.default_beam_search + sort_nbest behind Speech2Text.__call__, which the reference
 * builds with ESPnet's defaults (beam_size 20, search_type "default", score_norm, nbest 1, lm_weight 0:
 * pkg/espnet-asr/src/transcribe.py:27-31) and calls once per window (transcribe.py:68).  Graves' search: per frame, pop the
 * best open hypothesis, keep its blank extension, open its `beam` best label extensions, until `beam` kept hypotheses beat
 * everything still open.  The evaluation order is documented in oracle/espnet_beam.c and the results are bit-identical to it.
 *
 *   beam       beam_size (>= 1; clamped to the vocabulary)
 *   flags      RS_BEAM_SCORE_NORM: the winner is the best score / len(yseq) (yseq counts the leading blank), else the best score
 *   max_pops   prediction-network evaluations allowed per frame (0 = 16 * beam).  Upstream has no bound; a trained model needs
 *              about `beam` to 2 * beam.  The workspace grows with it.
 *   ids    i32[B][out_cap]  labels of the best hypothesis (no leading blank),  n_ids i32[B],  scores f32[B] (log-probability)
 *   frames i32[B][out_cap]  the encoder frame each label was appended at, or NULL ([UPSTREAM] NeMo keeps them as
 *                           Hypothesis.timestep; ESPnet's hypotheses carry none — the espnet package times its segments by CTC)
 *   pops   i32[B]           prediction-network evaluations spent on utterance b
 * Workspace: rs_rnnt_beam_workspace_bytes(ctx, B, beam, tp_max, max_pops), separate from rs_workspace_bytes.
 * Synchronises the stream internally.  RS_EOVERFLOW if a frame needed more than max_pops pops or a result has more than out_cap
 * labels (the affected rows return n_ids = 0). */
enum { RS_BEAM_SCORE_NORM = 1 };
size_t rs_rnnt_beam_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops);
int rs_rnnt_beam(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags,
                 int max_pops, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int32_t* pops,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- n-best lists from the default beam search — added within ABI 7 (probe the symbols) ------------------------------------------
 * replaces: `nbest=` of espnet2's Speech2Text, i.e. BeamSearchTransducer's `sort_nbest(kept_hyps)[:nbest]` at the end of the search,
 * which rs_rnnt_beam runs with nbest = 1.  The search is rs_rnnt_beam; what changes is what is read back after the last frame, inside
 * the step kernel — no further launch, no host round trip.
 * RANKING RULE, upstream's restated exactly.  The candidates are ALL hypotheses kept after the last frame — the survivors, at least
 * `beam` of them, in the kept list's order (ascending by score, ties in the order they were kept: oracle/espnet_beam.c).  They are
 * sorted by norm = score / len(yseq) with RS_BEAM_SCORE_NORM (yseq counts the leading blank; one float32 division), else by
 * norm = score, DESCENDING AND STABLE IN THE ORDER OF THE KEPT LIST, as Python's sorted(..., reverse=True) is: rank r is the first
 * maximum among those not yet ranked.  EQUAL LABEL SEQUENCES ARE NOT REMOVED, because upstream does not remove them (the same
 * labels reached along two alignments are two hypotheses of the kept list).  Entry 0 is bit for bit what rs_rnnt_beam returns.
 *   nbest             1..8 and <= beam (after the clamp to the vocabulary)
 *   ids / frames i32[B][nbest][out_cap]   labels (no leading blank) and the frame each was appended at (frames may be NULL), per entry
 *   n_ids i32[B][nbest]                   label count of each entry; an entry past n_hyps[b] has n_ids = 0 and is not otherwise specified
 *   scores f32[B][nbest]                  score (log-probability) of each entry, not normalised
 *   norm_scores f32[B][nbest]             the norm the entries are ranked by, descending
 *   n_hyps i32[B]                         nbest; 1 for an utterance without frames (its kept list is the start hypothesis: no labels,
 *                                         score 0); 0 for an utterance that overflowed max_pops
 * Workspace: rs_rnnt_beam_nbest_workspace_bytes (that of rs_rnnt_beam: the lists live in the outputs; 0 for invalid arguments or a
 * context that is not finalized).  Errors as rs_rnnt_beam; RS_EINVAL before anything is enqueued for nbest outside 1..8 or above the
 * beam; RS_EOVERFLOW if a frame needed more than max_pops pops or any returned entry has more than out_cap labels (that entry
 * returns n_ids = 0).  Restated by tests/espnet_beam_nbest_checker.c, which the lists equal bit for bit. */
size_t rs_rnnt_beam_nbest_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest);
int rs_rnnt_beam_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags,
                       int max_pops, int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                       float* norm_scores, int32_t* n_hyps, int32_t* pops, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sherpa-onnx's modified_beam_search (Zipformer family) ---------------------------------------
 * replaces: the search inside sherpa_onnx.OfflineRecognizer.from_transducer(..., decoding_method="modified_beam_search",
 * max_active_paths=K) — the second offline transducer method of the constructor the reference builds its recognizer with
 * (pkg/k2-asr/src/huggingface.py:73-83 passes "greedy_search" = rs_rnnt_greedy) — as model.decode_stream(stream) runs it
 * (pkg/k2-asr/src/transcribe.py:39).  [UPSTREAM, not vendored] OfflineTransducerModifiedBeamSearchDecoder::Decode without LM
 * (hotwords: rs_rnnt_mbs_hotwords below), Hypotheses::Add, GetMostProbable(length_norm):
 *   per utterance one starting hypothesis, ys = [-1, blank] (context_size = 2), log_prob = 0.  For every frame t < enc_lens[b]
 *   with the H <= K live hypotheses: logits[h] = output_linear(tanh(f[b][t] + decoder_proj(decoder(last 2 tokens of h))));
 *   logits[h][blank] -= blank_penalty; lp[h][v] = log_softmax(logits[h])[v] + log_prob[h]; the K largest of the H x V values
 *   (flat index h V + v) are taken in descending order: hypothesis h is copied, v is appended to ys and t to the timestamps
 *   unless v is the blank or <unk>, log_prob = lp[h][v]; a hypothesis whose ys equals one already in the new set (length and
 *   every token) is merged into it — log_prob = logaddexp(old, new), the tokens / timestamps of the one added first stay.
 *   Result: the hypothesis with the largest log_prob / len(ys) (len counts the 2 context entries).
 * Tie rules (upstream leaves them to a partial sort and an unordered map): equal values -> the lower flat index first;
 * equal final scores -> the hypothesis that entered the last set first.  All arithmetic is float32 in one order (upstream keeps
 * log_prob in double), stated in csrc/k_rnnt_mbs.hip and restated by tests/k2_mbs_checker.c, which the results equal bit for bit.
 *
 *   max_active_paths  K, 1..8 (1 = the greedy search's ids and frames)
 *   blank_penalty     >= 0, subtracted from the blank logit before the log-softmax
 *   flags             RS_MBS_LENGTH_NORM: the winner is the best log_prob / len(ys) (sherpa-onnx's default), else the best log_prob
 *   ids / frames i32[B][out_cap]  tokens of the winner (without the context) and the encoder frame of each
 *   n_ids i32[B],  scores f32[B]  log_prob of the winner, not normalised
 * Workspace: rs_rnnt_mbs_workspace_bytes(ctx, B, max_active_paths, tp_max, out_cap), separate from rs_workspace_bytes (0 for
 * invalid arguments).  The whole search is enqueued without a host round trip and the stream is synchronised once at the end.
 * RS_EOVERFLOW if a result has more than out_cap tokens; RS_EINVAL for a context without the stateless decoder (the search is
 * defined for the Zipformer family), max_active_paths outside 1..8 or a negative penalty. */
enum { RS_MBS_LENGTH_NORM = 1 };
size_t rs_rnnt_mbs_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap);
int rs_rnnt_mbs(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---- hotwords (contextual biasing) in the modified beam search — added within ABI 7 ---------------
 * replaces: the `hotwords_file=` / `hotwords_score=` keywords of sherpa_onnx.OfflineRecognizer.from_transducer and
 * `create_stream(hotwords=...)`, as the modified_beam_search applies them.  [UPSTREAM, not vendored, PARITY UNPINNED]
 * sherpa-onnx's ContextGraph (Build, FillFailOutput, ForwardOneStep(strict_mode = false), Finalize) and its use in
 * OfflineTransducerModifiedBeamSearchDecoder::Decode, restated:
 *   graph: a trie over the token ids of the phrases; root: token -1, level 0, node_score 0, fail = root.  Phrase i has score s_i.
 *   A token that creates a node: token_score = s_i, node_score = parent.node_score + s_i; a token that meets a node:
 *   token_score = max(s_i, token_score), node_score = parent.node_score + token_score; both: is_end |= (last token of the phrase),
 *   output_score = is_end ? node_score : 0.  Fail links breadth-first (children of the root fail to the root; child c of cur on
 *   token t: follow f = cur.fail, f.fail, ... to the first node with a child on t — that child — else the root); c.output = the
 *   first is_end node on c.fail, c.fail.fail, ... before the root (none otherwise), c.output_score += c.output.output_score.
 *   step(state, token) -> (delta, next):  state has a child n on the token: score = n.token_score.  Otherwise n = state.fail;
 *   while n has no child on the token: n = n.fail, stop at the root; n = that child if there is one;
 *   score = n.node_score - state.node_score.  n.output_score != 0 (the non-strict exit): out = n.is_end ? n.node_score :
 *   n.output ? n.output.node_score : n.node_score; delta = (score + out) - n.node_score, next = root.  Otherwise
 *   delta = score + n.output_score, next = n.
 *   Finalize(state): delta = -state.node_score.
 *   in the search (steps 4 - 5 of rs_rnnt_mbs): the starting hypothesis of an utterance with a graph carries context_state = the
 *   graph's root.  The K best of the H x V values are selected as in rs_rnnt_mbs, WITHOUT any bonus.  A selected candidate that
 *   appends a label v: (delta, state') = step(parent.context_state, v), log_prob = lp[h][v] + delta, context_state = state'; one
 *   that appends nothing keeps its parent's state.  Merging as in rs_rnnt_mbs (logaddexp of the log_probs with their bonuses); the
 *   tokens, timestamps AND context state of the one added first stay.  After the utterance's last frame every hypothesis of the
 *   final set gets log_prob += -node_score(context_state); then the winner is chosen, by the rule and tie rule of rs_rnnt_mbs.
 *   scores[b] = the winner's log_prob after that.  An utterance without a graph is searched exactly as by rs_rnnt_mbs.
 * All numbers float32 in the order csrc/k_rnnt_mbs.hip states and tests/k2_mbs_checker.c restates (bit for bit); scores that
 * are multiples of 0.5 make every graph quantity exact.
 *
 * rs_hotwords: the graphs of a call as flat arrays, all graphs concatenated (node and child indices are global):
 *   child_begin i32[n_nodes + 1]   CSR: the children of node n are the entries child_begin[n] .. child_begin[n + 1] - 1 of
 *   child_tok / child_node i32[n_children]   token (ascending within a node) and node of each child
 *   fail i32[n_nodes], output i32[n_nodes] (-1 = none), is_end i32[n_nodes] (0 / 1), level i32[n_nodes] (depth in the trie)
 *   token_score / node_score / output_score f32[n_nodes]
 *   graph_root i32[n_graphs]       root node of graph g;   max_level = the largest level
 * rs_rnnt_mbs_hotwords reads DEVICE pointers; rs_hotwords_host is the same layout with HOST pointers, for rs_hotwords_check.
 *   graph_of i32[B] (device)       graph of utterance b, -1 = none
 * Every walk on the device is a counted loop (at most max_level + 1 fail steps, 32 bisection steps) and an index outside the
 * table is treated as the root and never dereferenced: a corrupt table may give a wrong bonus, it cannot spin or read out of
 * bounds.  rs_hotwords_check (pure host code, no context) validates a table before upload: counts, index ranges, children
 * sorted strictly ascending, roots at level 0 that fail to themselves, level[child] = level[parent] + 1,
 * level[fail[n]] < level[n] for every other node, level <= max_level; RS_EINVAL with the reason in msg (msg_bytes, may be NULL).
 * rs_rnnt_mbs_hotwords with hw == NULL, n_graphs == 0 or graph_of == NULL is rs_rnnt_mbs (the same kernels, the same bits);
 * otherwise the hotword form of the selection kernel runs: still five launches per frame, nothing waits for the host, one
 * synchronisation at the end.  Workspace: rs_rnnt_mbs_hotwords_workspace_bytes.  Errors as rs_rnnt_mbs, and RS_EINVAL for
 * negative counts or null arrays. */
typedef struct rs_hotwords {
    const int32_t* child_begin;
    const int32_t* child_tok;
    const int32_t* child_node;
    const int32_t* fail;
    const int32_t* output;
    const int32_t* is_end;
    const int32_t* level;
    const float* token_score;
    const float* node_score;
    const float* output_score;
    const int32_t* graph_root;
    int32_t n_nodes, n_children, n_graphs, max_level;
} rs_hotwords;
typedef rs_hotwords rs_hotwords_host;
int rs_hotwords_check(const rs_hotwords_host* table, char* msg, size_t msg_bytes);
size_t rs_rnnt_mbs_hotwords_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap);
int rs_rnnt_mbs_hotwords(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                         float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids,
                         float* scores, const rs_hotwords* hw, const int32_t* graph_of, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- n-gram language model shallow fusion in the modified beam search — added within ABI 7 (probe the symbols) ----------------
 * [UPSTREAM, not vendored, UNVERIFIED] icefall's modified_beam_search_lm_shallow_fusion / modified_beam_search_ngram_rescoring
 * add an n-gram LM's score to a hypothesis after the top-K pick of a frame; the slot below is believed to be theirs and has not
 * been compared with them.  sherpa-onnx's own `lm=` / `lm_scale=` is a neural LM and is not this.
 * The model is an rs_ngram and the step is `step` of rs_ngram, both stated with rs_rnnt_alsd_lm below, unchanged.  The search is
 * rs_rnnt_mbs / rs_rnnt_mbs_hotwords with these additions:
 *   every hypothesis row carries an LM state; the starting hypothesis stands at lm.start (an index outside the nodes counts as
 *   the root).  Steps 1 - 4 are unchanged: the K best of the H x V values are selected WITHOUT the LM term and without any
 *   hotword bonus.  The LM therefore re-ranks only among the K survivors of a frame and acts on later frames through log_prob; it
 *   cannot rescue a candidate that was not selected.  THIS DIFFERS FROM rs_rnnt_alsd_lm ON PURPOSE: there the LM term is part of
 *   the value the pruning ranks, here it is added after the selection.
 *   Step 5, before the merge: a selected candidate that appends a label v (neither the blank nor <unk>) from a parent with LM
 *   state s is scored, float32, no contraction, in this order:
 *       lp = lp[h][v];   with a graph: lp = lp + delta (as rs_rnnt_mbs_hotwords);   (l, s') = step(s, v);
 *       log_prob = lp + (lm_alpha * l)        the product is rounded first
 *   and its LM state is s'.  A candidate that appends nothing (blank or <unk>) keeps its score and state and makes no walk.
 *   The merge is unchanged: rs_logaddexpf of the log_probs with their terms inside; tokens, timestamps, context state and LM
 *   state of the entry added first stay (equal token sequences have equal LM states anyway).  No end-of-sentence term.  The
 *   hotword Finalize at the last frame is unchanged and is applied to the LM-inclusive score before the winner is chosen.
 *   scores[b] includes the LM terms; rs_rnnt_token_scores keeps reporting the model's unmodified distribution.
 * rs_rnnt_mbs_lm with lm == NULL, lm->n_nodes == 0 or lm_alpha == 0 is rs_rnnt_mbs_hotwords (the same kernels, the same bits;
 * with no graphs as well, rs_rnnt_mbs).  Otherwise the LM form of the selection kernel runs, which carries the call's graphs or
 * none: still five launches per frame, nothing waits for the host, one synchronisation at the end.  Workspace:
 * rs_rnnt_mbs_lm_workspace_bytes, the hotword layout plus one LM state per hypothesis row, twice (0 for invalid arguments or a
 * context that is not finalized).  Errors as rs_rnnt_mbs_hotwords, and RS_EINVAL before anything is enqueued for an lm_alpha
 * that is negative or not finite, lm->n_logits other than the context's, order outside 1..8, start outside the nodes, negative
 * counts or null arrays. */
struct rs_ngram;
size_t rs_rnnt_mbs_lm_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap);
int rs_rnnt_mbs_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                   float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                   const rs_hotwords* hw, const int32_t* graph_of, const struct rs_ngram* lm, float lm_alpha, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- n-best lists from the modified beam search — added within ABI 7 (probe the symbols) ----------------------------------------
 * The project's addition: sherpa-onnx returns one hypothesis per stream and has no n-best option.  The search is rs_rnnt_mbs_lm
 * (hw, graph_of and lm may each be NULL, lm_alpha may be 0: then the hotword or the plain form runs, as there); what changes is what
 * is read from the last set, inside the selection kernel of the utterance's last frame — no further launch, no host round trip.
 * RANKING RULE.  The candidates are the hypotheses of the set the last frame leaves, after merging and after the hotword Finalize,
 * in the order in which they entered that set.  Each has norm = log_prob / len(ys) with RS_MBS_LENGTH_NORM (len counts the 2
 * context entries, one float32 division) and norm = log_prob without it.  Rank r holds the candidate with the greatest norm among
 * those not yet ranked; EQUAL NORMS: THE ONE THAT ENTERED THE LAST SET FIRST — rs_rnnt_mbs's rule and tie rule applied down the
 * list, so entry 0 is bit for bit what rs_rnnt_mbs / _hotwords / _lm return for the same arguments.  Equal token sequences cannot
 * occur twice: the set merged them.
 *   nbest             1..8 and <= max_active_paths
 *   ids / frames i32[B][nbest][out_cap]   tokens (without the context) and the encoder frame of each, per entry
 *   n_ids i32[B][nbest]                   token count of each entry; an entry past n_hyps[b] has n_ids = 0 and is not otherwise specified
 *   scores f32[B][nbest]                  log_prob of each entry, not normalised, after Finalize (what scores[b] of rs_rnnt_mbs_lm carries)
 *   norm_scores f32[B][nbest]             the norm the entries are ranked by, descending
 *   n_hyps i32[B]                         min(nbest, size of the last set); 0 for an utterance without frames
 * Workspace: rs_rnnt_mbs_nbest_workspace_bytes (the layout of rs_rnnt_mbs_lm: the lists live in the outputs; 0 for invalid arguments
 * or a context that is not finalized).  Errors as rs_rnnt_mbs_lm; RS_EINVAL before anything is enqueued for nbest outside 1..8 or
 * above max_active_paths; RS_EOVERFLOW if any returned entry has more than out_cap tokens.  Restated by
 * tests/k2_mbs_nbest_checker.c, which the lists equal bit for bit. */
size_t rs_rnnt_mbs_nbest_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap, int nbest);
int rs_rnnt_mbs_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                      float blank_penalty, int flags, int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids,
                      float* scores, float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of,
                      const struct rs_ngram* lm, float lm_alpha, void* workspace, size_t workspace_bytes, void* stream);

/* ---- hotwords (contextual biasing) in the ALSD beam search — added within ABI 7 ---------------------
 * gives the LSTM transducers (the NeMo family: FastConformer-RNNT, whose checkpoint ships `strategy: alsd`) what
 * rs_rnnt_mbs_hotwords gives the Zipformer family.  [UPSTREAM] NeMo's align_length_sync_decoding has no hotword rule: the
 * semantics are this project's.  The graph (rs_hotwords, graph_of), `step` and `Finalize` are the ones stated above for
 * rs_rnnt_mbs_hotwords; the search is rs_rnnt_alsd with these additions for an utterance b whose graph_of[b] >= 0:
 *   every hypothesis carries a context_state, a node of its utterance's graph; the start hypothesis stands at the graph's root.
 *   expansion of a hypothesis with score hs and state s: the `beam` best non-blank tokens are picked by raw logit as in
 *   rs_rnnt_alsd.  The blank candidate is unchanged: hs + (z[blank] - lse), state s.  A label candidate v takes
 *   (delta, s') = step(s, v); its score is (hs + (z[v] - lse)) + delta, in that float32 order, its state s'.
 *   selection of the `beam` best candidates RANKS THE BOOSTED SCORES, ties as in rs_rnnt_alsd (the lower candidate index first).
 *   This differs from rs_rnnt_mbs_hotwords on purpose: there the bonus is added after the selection, here it is part of the
 *   ranking, so a phrase continuation inside its hypothesis's top `beam` can overtake.  Recombination is unchanged: equal label
 *   sequences have equal states by construction, and the first occurrence's state stays.
 *   a hypothesis recorded as finished (a blank taken at the last frame) is recorded with sc + (-node_score(state)) (Finalize),
 *   sc its score after recombination; the normalised score compared with the best so far is computed from that value.  The
 *   "nothing finished: the best of the beam" exit applies the same Finalize to every beam entry before comparing.
 *   scores[b] = the winner's score including its net bonus.  A new hypothesis's state is its candidate's state.
 * An utterance without a graph inside a hotword call yields the bits of rs_rnnt_alsd.  All numbers float32 in the order
 * csrc/k_rnnt_alsd.hip states and tests/alsd_checker.c restates (bit for bit); scores that are multiples of 0.5 make
 * every graph quantity exact.  The walk on the device is the one of rs_rnnt_mbs_hotwords (csrc/k_rnnt_hotwords.h): counted loops
 * only, an index outside the table is the root and is never dereferenced; validate a table with rs_hotwords_check before upload.
 * rs_rnnt_alsd_hotwords with hw == NULL, n_graphs == 0 or graph_of == NULL launches the plain kernels of rs_rnnt_alsd (the same
 * bits); otherwise the hotword form of the selection kernel runs: still six launches per alignment step, no further host round
 * trip.  Workspace: rs_rnnt_alsd_hotwords_workspace_bytes, the plain layout plus one state per hypothesis row (0 for invalid
 * arguments or a context that is not finalized).  Errors as rs_rnnt_alsd, and RS_EINVAL for negative counts or null arrays;
 * RS_EINVAL for a Zipformer or AV-HuBERT context.  rs_rnnt_token_scores on the result reports the model's unmodified
 * distribution (no bonus). */
size_t rs_rnnt_alsd_hotwords_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio,
                                             int max_target_abs);
int rs_rnnt_alsd_hotwords(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                          double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids,
                          int32_t* steps, int32_t* n_ids, float* scores, const rs_hotwords* hw, const int32_t* graph_of,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- n-gram language model (shallow fusion) in the ALSD beam search — added within ABI 7 -------------
 * gives the NeMo family what `decoding.beam.ngram_lm_model` / `ngram_lm_alpha` give upstream: a backoff n-gram model, trained on
 * the user's own text, whose log-probability of every label expansion enters the ranking.  [UPSTREAM, not vendored, UNVERIFIED]
 * NeMo's align_length_sync_decoding is believed to add ngram_lm_alpha * lm_score to each of a hypothesis's top-k expansions after
 * the top-k pick (NeMo is not available to this project); that is the slot rs_rnnt_alsd_hotwords already ranks in, and the rule
 * below is stated for it.  No end-of-sentence term: upstream ALSD adds none, and the search never emits `</s>`.
 *
 * rs_ngram: one model as flat arrays, natural logarithms (each value = float32(log10 value x ln 10), the product in float64):
 *   child_begin i32[n_nodes + 1]   CSR over a forward trie of token ids; node 0 is the root (the empty context)
 *   child_tok / child_node i32[n_children]   token (strictly ascending within a node) and node of each child
 *   root_child i32[n_logits]       node of the unigram of token v, -1 = none (most walks end here: one load, not a bisection)
 *   logp / backoff f32[n_nodes]    of the node's n-gram; backoff 0 where the file gives none
 *   suffix i32[n_nodes]            node of the longest proper suffix of the node's words that the model has; the root's is the root
 *   level i32[n_nodes]             n-gram length; root 0
 *   start                          node of `<s>` if the model has it (a level-1 node in no child list: no token reaches it), else 0
 *   order                          the model's order, 1..8;   unk_logp = `<unk>`'s log-probability (or the model's lowest unigram's)
 * rs_rnnt_alsd_lm reads DEVICE pointers; rs_ngram_host is the same layout with HOST pointers, for rs_ngram_check.
 *   step(state s, token v) -> (lp, next), float32, no contraction:
 *     n = s; acc = 0; c = none
 *     repeat at most order + 1 times:
 *         c = (n == root) ? root_child[v] : child(n, v)             (bisection, at most 32 steps)
 *         if c found or n == root: stop
 *         acc = acc + backoff[n]; n = suffix[n]
 *     found:      lp = acc + logp[c];   next = level[c] < order ? c : suffix[c]
 *     not found:  lp = acc + unk_logp;  next = root
 *   in the search (rs_rnnt_alsd / rs_rnnt_alsd_hotwords with these additions): every hypothesis row carries an LM state; the start
 *   hypothesis stands at `start`.  The blank candidate is unchanged and keeps the state.  A label candidate v of a hypothesis with
 *   score hs and state s: cs = hs + (z[v] - lse); with a hotword graph on that utterance cs = cs + delta exactly as in
 *   rs_rnnt_alsd_hotwords; then (lp, s') = step(s, v) and cs = cs + (lm_alpha * lp), the product rounded first; its LM state is s'.
 *   Selection ranks these scores, ties as in rs_rnnt_alsd.  Recombination is unchanged (the state is a function of the label
 *   sequence alone) and the first occurrence's state stays.  scores[b] includes the LM terms; rs_rnnt_token_scores keeps reporting
 *   the model's unmodified distribution.
 * All numbers float32 in the order csrc/k_rnnt_alsd.hip / csrc/k_rnnt_ngram.h state and tests/alsd_checker.c restates (bit for
 * bit).  Every walk on the device is a counted loop (order + 1 backoff steps, 32 bisection steps); a node or child index outside
 * the table is replaced by the root before it is used and a token outside root_child counts as not found: a corrupt table can give
 * a wrong score and nothing else.  rs_ngram_check (pure host code, no context) validates a table before upload: counts and index
 * ranges, children strictly ascending, level[child] = level[parent] + 1, level[suffix[n]] < level[n] for every node but the root,
 * every root_child entry a level-1 child of the root on that token, `start` the root or a level-1 node, every value finite;
 * RS_EINVAL with the reason in msg (msg_bytes, may be NULL).
 * rs_rnnt_alsd_lm with lm == NULL, n_nodes == 0 or lm_alpha == 0 is rs_rnnt_alsd_hotwords (the same kernels, the same bits; with
 * hw == NULL as well that is rs_rnnt_alsd); otherwise the LM form of the selection kernel runs, candidate j's walk on lane j of
 * its hypothesis's wave: still six launches per alignment step, no further host round trip.  Workspace:
 * rs_rnnt_alsd_lm_workspace_bytes, the hotword layout plus one LM state per hypothesis row, twice (0 for invalid arguments or a
 * context that is not finalized).  Errors as rs_rnnt_alsd_hotwords, and RS_EINVAL, before anything is enqueued, for negative counts
 * or null arrays, a non-finite or negative lm_alpha, lm->n_logits different from the context's, `order` outside 1..8, `start`
 * outside the nodes; RS_EINVAL for a Zipformer or AV-HuBERT context. */
typedef struct rs_ngram {
    const int32_t* child_begin;
    const int32_t* child_tok;
    const int32_t* child_node;
    const int32_t* root_child;
    const float* logp;
    const float* backoff;
    const int32_t* suffix;
    const int32_t* level;
    int32_t n_nodes, n_children, n_logits, order, start;
    float unk_logp;
} rs_ngram;
typedef rs_ngram rs_ngram_host;
int rs_ngram_check(const rs_ngram_host* table, char* msg, size_t msg_bytes);
size_t rs_rnnt_alsd_lm_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs);
int rs_rnnt_alsd_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                    double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids, int32_t* steps,
                    int32_t* n_ids, float* scores, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm,
                    float lm_alpha, void* workspace, size_t workspace_bytes, void* stream);

/* ---- n-best lists from the ALSD beam search — added within ABI 7 (probe the symbols) ---------------------------------------------
 * replaces: NeMo's beam decoding with `return_best_hypothesis=False` (NBestHypotheses), i.e. `sort_nbest(final)` at the end of
 * align_length_sync_decoding, with equal label sequences removed.  The search is rs_rnnt_alsd_lm (hw, graph_of and lm may each be
 * NULL, lm_alpha may be 0: then the hotword or the plain form runs, as there); in place of the single best finished hypothesis the
 * selection kernel keeps `nbest` ranked ones per utterance during the search — no further launch, no host round trip.
 * RANKING RULE.  Entry condition, score and norm are exactly rs_rnnt_alsd's: a blank taken at the utterance's last frame finishes a
 * hypothesis; its score is read after this step's recombination; under hotwords the value is sc + (-node_score(state)) (Finalize);
 * norm = sc / (n + 1) with RS_ALSD_SCORE_NORM (n labels; one float32 division), else norm = sc.  A candidate ENTERS BELOW EVERY
 * ENTRY WHOSE NORM IS >= ITS OWN, so the earlier-finished one wins ties, as rs_rnnt_alsd's strict `>` does; a full list drops its
 * last entry.  THE LIST HOLDS EACH LABEL SEQUENCE AT MOST ONCE: equal sequences can only finish in the same alignment step
 * (i = T - 1 + n), which happens when RS_ALSD_MERGE is off and recombined duplicates stay in the beam; of those the one with the
 * greater norm is kept, and the one considered first (the lower beam slot) on a tie.  The list is therefore NeMo's
 * sort_nbest(final)[:nbest] with duplicates removed, and entry 0 is bit for bit what rs_rnnt_alsd / _hotwords / _lm return.
 * When nothing finished (alignment budget spent, or no frames), the list is the beam's entries under the same ranking and
 * de-duplication, each after Finalize — rs_rnnt_alsd's exit already ranks them.
 *   nbest             1..8 and <= beam (after the clamp to the vocabulary)
 *   ids / steps i32[B][nbest][out_cap]    labels and the alignment step of each, per entry
 *   n_ids i32[B][nbest]                   label count of each entry; an entry past n_hyps[b] has n_ids = 0 and is not otherwise specified
 *   scores f32[B][nbest]                  the score of each entry, not normalised, after Finalize (what scores[b] of rs_rnnt_alsd_lm carries)
 *   norm_scores f32[B][nbest]             the norm the entries are ranked by, descending
 *   n_hyps i32[B]                         entries valid for utterance b, 1..nbest (an utterance without frames: 1, the empty start hypothesis)
 * Labels move at most once per insertion: a slot table with an order array (the ranks hold slot numbers); one wave does the insert
 * with the label copy spread over its lanes.  Workspace: rs_rnnt_alsd_nbest_workspace_bytes (the layout of rs_rnnt_alsd_lm plus
 * 8 label slots per utterance; 0 for invalid arguments or a context that is not finalized).  Errors as rs_rnnt_alsd_lm; RS_EINVAL
 * before anything is enqueued for nbest outside 1..8 or above the beam; RS_EOVERFLOW if any returned entry has more than out_cap
 * labels.  Restated by tests/alsd_nbest_checker.c, which the lists equal bit for bit. */
size_t rs_rnnt_alsd_nbest_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs,
                                          int nbest);
int rs_rnnt_alsd_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                       double max_target_ratio, int max_target_abs, int flags, int nbest, int out_cap, int32_t* ids, int32_t* steps,
                       int32_t* n_ids, float* scores, float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw,
                       const int32_t* graph_of, const rs_ngram* lm, float lm_alpha, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- hotwords and n-gram LM fusion in the default beam search — added within ABI 7 (probe the symbols) ---------------------------
 * gives the espnet package what rs_rnnt_alsd_hotwords / _lm give nemo and rs_rnnt_mbs_hotwords / _lm give k2: contextual biasing
 * from a phrase list (rs_hotwords, stated with rs_rnnt_mbs_hotwords) and shallow fusion of a backoff n-gram model (rs_ngram, stated
 * with rs_rnnt_alsd_lm), with the tables, `step` and `finalize` of those entries unchanged.
 * [UPSTREAM, not vendored, UNVERIFIED] espnet2 BeamSearchTransducer.default_beam_search with an LM: `beam_logp, beam_idx =
 * logp[1:].topk(beam_k)` is taken first, then every label extension k it opens gets `score + beam_logp + lm_weight * lm_scores[k + 1]`
 * — the slot the reference closes with lm_weight = 0.  (ESPnet cannot run here: the rule is restated from its source text.)  The
 * hotword rule is this project's own: ESPnet's transducer search has none.
 * The search is rs_rnnt_beam with these additions.  Every hypothesis carries an LM state and — for an utterance b with
 * graph_of[b] >= 0 — a context state; both are functions of its label sequence alone.  The start hypothesis [blank] stands at
 * lm->start and at its graph's root.  Popping a hypothesis with score hs, LM state s and context state c:
 *   - the record of its joint row is unchanged: the beam_k best labels are picked by raw logit WITHOUT any term;
 *   - the blank extension is unchanged: kept with hs + logp(blank), states s and c;
 *   - a label extension v is scored in float32 without contraction, in this order:
 *         sc = hs + logp(v);   with a graph: (delta, c') = step(c, v), sc = sc + delta;
 *         with an LM: (lp, s') = step(s, v), sc = sc + (lm_alpha * lp), the product rounded first;
 *     and enters the open list with sc, s', c'.  The open list ranks sc: the terms decide the pop order and the end-of-frame test
 *     (`beam` kept scores strictly above the open list's maximum).
 * After the last frame the survivors keep the kept list's order (ascending by score BEFORE Finalize, ties in kept order); each gets
 * sc = sc + (-node_score(c)) (Finalize: a phrase left open gives its bonus back); only then norm = sc / len(yseq) (or sc) is formed
 * and the winner / the n-best ranking is today's.  scores and norm_scores carry the values after Finalize, the LM terms inside.
 * There is no end-of-sentence term.  rs_rnnt_token_scores keeps reporting the model's unmodified distribution.
 *   nbest             0: the outputs of rs_rnnt_beam (ids / frames [B][out_cap], n_ids / scores [B]; norm_scores and n_hyps may be
 *                     NULL);   1..8 and <= beam: the lists and the ranking of rs_rnnt_beam_nbest
 *   hw, graph_of, lm, lm_alpha   as rs_rnnt_alsd_lm takes them (DEVICE pointers)
 * With hw == NULL, hw->n_graphs == 0 or graph_of == NULL, AND lm == NULL, lm->n_nodes == 0 or lm_alpha == 0, the plain kernels run:
 * the instantiation and the bits of rs_rnnt_beam / rs_rnnt_beam_nbest.  An utterance without a graph inside a hotword call gets the
 * bits of the plain search.  Positive bonuses let an extension outscore its parent, so a frame can need more pops than the plain
 * search: RS_EOVERFLOW stays the answer.
 * Errors as rs_rnnt_beam; RS_EINVAL before anything is enqueued for a Zipformer or AV-HuBERT context, a negative or non-finite
 * lm_alpha, lm->n_logits other than the context's, order outside 1..8, start outside the nodes, negative counts or null arrays in
 * either table, nbest outside 0..8 or above the beam.  Workspace: rs_rnnt_beam_lm_workspace_bytes (the layout of rs_rnnt_beam plus a
 * context state and an LM state per open-list and kept entry; 0 for invalid arguments or a context that is not finalized).
 * Restated in all its forms by tests/espnet_beam_lm_checker.c, which the results equal bit for bit. */
size_t rs_rnnt_beam_lm_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest);
int rs_rnnt_beam_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags,
                    int max_pops, int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                    float* norm_scores, int32_t* n_hyps, int32_t* pops, const rs_hotwords* hw, const int32_t* graph_of,
                    const rs_ngram* lm, float lm_alpha, void* workspace, size_t workspace_bytes, void* stream);

/* ---- token log-probabilities of a finished transducer search — added within ABI 7 ----------------
 * gives what NeMo's Hypothesis.token_confidence (preserve_token_confidence, method max_prob), sherpa-onnx's per-token log-probs
 * and ESPnet's scored hypotheses give: how sure the model was of every token it emitted.  A teacher-forced pass over the OUTPUT
 * of any search of this header (rs_rnnt_greedy, rs_rnnt_alsd / _hotwords, rs_rnnt_beam, rs_rnnt_mbs / _hotwords); it runs after the search,
 * shares none of its kernels' state and leaves ids / frames / n_ids as they are.  For token u of utterance b, emitted at frame t:
 *     logp[b][u] = z[id] - logsumexp(z),   z = W_out . act(f[b][t] + g(y_<u)) + b_out
 * with g(y_<u) the prediction network's output after the start context and the first u labels: the model's unmodified
 * distribution (no blank penalty, no hotword bonus).  top1[b][u] = argmax_v z[v], the lowest index on ties, as the searches break
 * them: for a greedy result top1 == ids; a beam search may have kept a token that was not the row's best.  Float32 in one order
 * (the prediction network and logits of the searches, the log-sum-exp of oracle/rnnt_alsd.c), stated in csrc/k_rnnt_scores.hip
 * and restated by tests/token_scores_checker.c, which the results equal bit for bit; a row's bits depend neither on the rest of
 * the batch nor on the workspace given.
 *
 *   joint_enc, enc_lens, B, tp_max   what the search read
 *   ids / frames i32[B][u_cap], n_ids i32[B]   what the search wrote (u_cap = its u_max / out_cap: the row pitch)
 *   flags    RS_SCORES_FRAMES_ARE_STEPS: `frames` holds alignment steps (rs_rnnt_alsd: frame = step - index), converted on the
 *            device; rs_rnnt_greedy, rs_rnnt_beam and rs_rnnt_mbs write frames: no flag
 *   logp     f32[B][u_cap];  top1 i32[B][u_cap] or NULL.  Slots at u >= n_ids[b] are left untouched.
 * Workspace: rs_rnnt_token_scores_workspace_bytes(ctx, B, u_cap) is the MINIMUM, separate from rs_workspace_bytes (0 for invalid
 * arguments).  The (b, u) rows, compacted in (b, u) order, are scored in chunks: the minimum holds 32 rows per chunk, every
 * further 32 rows cost 32 x 4 x (joint_hidden + 64 ceil(n_logits / 64)) bytes (+ the decoder rows of a Zipformer context), and a
 * workspace that holds all B x u_cap rows makes one chunk.  Same bits whatever the chunk.
 * Synchronises the stream internally (twice: the row count comes back first).  RS_EINVAL — before anything is enqueued — for an
 * AV-HuBERT or unfinalised context, a negative size, an unknown flag, a null pointer or a workspace below the minimum.  The
 * kernels check every frame against enc_lens (and tp_max), every id against n_logits and every count against u_cap before they
 * index anything: a bad entry puts NaN (top1 -1) in its slot and the call returns RS_EINVAL after the sync; nothing is read or
 * written out of range. */
enum { RS_SCORES_FRAMES_ARE_STEPS = 1 };
size_t rs_rnnt_token_scores_workspace_bytes(const rs_ctx* ctx, int B, int u_cap);
int rs_rnnt_token_scores(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                         const int32_t* frames, const int32_t* n_ids, int u_cap, int flags, float* logp, int32_t* top1,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- forced alignment and transcript likelihood on the transducer lattice — added within ABI 7 ----
 * answers what the reference's corpus tools ask of a model (pkg/_v1/src/align.py, pkg/espnet-oneseg: align a known text to the
 * audio, keep or drop the utterance by its score) for the families without a CTC head: here is a text, how well does it fit this
 * audio, and when was each token spoken?  The transducer lattice of Graves 2012.  For utterance b, T = min(enc_lens[b], tp_max),
 * labels y_1..y_U (U = n_ids[b]), g(u) the prediction network's output after the start context and the first u labels (u = 0..U),
 *     z(t,u) = W_out . act(f[b][t] + g(u)) + b_out,   lb(t,u) = z[blank] - lse(z),   ly(t,u) = z[y_(u+1)] - lse(z)   (u < U)
 * in the float32 order of rs_rnnt_token_scores: ly(t,u) is, bit for bit, what that entry returns for token u placed at frame t.
 *   no flag (NeMo, ESPnet)    a(0,0) = 0;  a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t,u-1) + ly(t,u-1));  loglik = a(T-1,U) + lb(T-1,U)
 *   RS_ALIGN_ONE_PER_FRAME    a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t-1,u-1) + ly(t-1,u-1)) over t = 0..T;  loglik = a(T,U): a label
 *                             also advances the frame, as every Zipformer search of this header moves; feasible only for U <= T
 *   lae(a, b)                 m = max(a, b); -inf when m is -inf, else m + log(exp(a - m) + exp(b - m)) (the searches' exp and
 *                             log); a is the blank term; a predecessor outside the lattice contributes -inf
 *   loglik f32[B]             log P(text | audio), the sum over all alignments
 *   best f32[B]               the same recursion with max in place of lae: the Viterbi score; ties go to the blank predecessor
 *   frames i32[B][u_cap]      frame at which label u + 1 is emitted on that path: non-decreasing, strictly increasing with the flag
 *   logp f32[B][u_cap]        ly(frames[b][u], u)
 * Rows that are no error: T = 0 and U = 0 give loglik = best = 0; an infeasible row (T = 0 with U > 0, or U > T with the flag)
 * gives loglik = best = -inf, frames -1 and logp NaN.  Slots at u >= n_ids[b] are left untouched.
 * u_cap (the row pitch of ids, frames and logp) is at most RS_ALIGN_U_CAP_MAX.
 * Workspace: rs_rnnt_align_workspace_bytes(ctx, B, tp_max, u_cap) is the MINIMUM (0 for invalid arguments); it holds the whole
 * lattice (two floats and a back-pointer bit per cell of B x tp_max x (u_cap + 1)) and 32 lattice rows of joint logits per
 * chunk; every further 32 rows per chunk cost what they cost rs_rnnt_token_scores.  Same bits whatever the chunk and whatever
 * else is in the batch; stated in csrc/k_rnnt_align.hip and restated serially by tests/rnnt_align_checker.c.
 * Synchronises the stream internally (twice).  RS_EINVAL — before anything is enqueued — for an AV-HuBERT or unfinalised context,
 * a null pointer, a negative size, an unknown flag, u_cap above the bound or a workspace below the minimum.  The kernels check
 * every count against u_cap and every id against the vocabulary before they index anything, and the blank id is no label: a bad
 * entry makes its row's loglik / best / logp NaN and its frames -1, the call returns RS_EINVAL after the sync and the other rows
 * keep their bits; nothing is read or written out of range. */
enum { RS_ALIGN_ONE_PER_FRAME = 1 };
#define RS_ALIGN_U_CAP_MAX 2047
size_t rs_rnnt_align_workspace_bytes(const rs_ctx* ctx, int B, int tp_max, int u_cap);
int rs_rnnt_align(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                  const int32_t* n_ids, int u_cap, int flags, float* loglik, float* best, int32_t* frames, float* logp,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- several texts per utterance on one lattice (n-best rescoring by full likelihood) — added within ABI 7 ----
 * rs_rnnt_align over R text rows that share the B utterances: row r is scored against the frames of utterance row_utt[r], and the
 * lattice cells that rows of one utterance have in common — the columns of a shared label prefix — are computed once.
 *   joint_enc, enc_lens, B, tp_max   the utterances, as for rs_rnnt_align
 *   row_utt i32[R] (device)   utterance of row r; -1: the row is skipped and NONE of its output slots is touched.  The non-negative
 *                             entries are non-decreasing, below B, and at most RS_ALIGN_ROWS_PER_UTT_MAX rows name one utterance.
 *   ids i32[R][u_cap], n_ids i32[R]; loglik / best f32[R]; frames i32 / logp f32 [R][u_cap]   per row, as rs_rnnt_align's per utterance
 *   flags    RS_ALIGN_ONE_PER_FRAME as above; RS_ALIGN_NO_SHARING: every row computes its whole lattice (the same bits; for A/B)
 *   stats    host int64_t[2] or NULL, filled after the internal sync: [0] lattice rows whose joint was computed, [1] lattice rows
 *            there are without sharing, the sum of T_r (U_r + 1) over the rows with a lattice
 * THE SHARING RULE.  A row has a lattice as above: not skipped, not bad, T > 0, and U <= T with one label per frame.  For a row r
 * with a lattice, over the earlier rows r' < r of the same utterance that have a lattice: m(r) = the greatest number of leading
 * labels r has in common with one of them, donor(r) = the first row that attains it; without such a row m(r) = 0 and there is no
 * donor (nor is there one at m = 0: nothing would be read from it).  Row r computes its cells with u >= m(r) — column m(r) again,
 * because ly(t, m) picks another label from the same logits — and reads the cells with u < m(r) from its donor, through the donor's
 * own donor where u < m(donor): a chain at most RS_ALIGN_ROWS_PER_UTT_MAX - 1 deep.  So stats[0] = sum of T_r (U_r + 1 - m(r)).
 * A bad or infeasible row is never a donor.  The rule is stated in csrc/rs_align_rows_plan.h (pure integers, also built alone on the
 * host by the tests).
 * THE GUARANTEE.  loglik, best, frames and logp of row r equal, bit for bit, what rs_rnnt_align returns for a batch of R utterances
 * whose row r holds a copy of utterance row_utt[r]'s joint_enc frames and enc_lens — with and without RS_ALIGN_NO_SHARING, whatever
 * the chunk and whatever else is in the batch: a cell's bits depend on the utterance, the frame and the label prefix only.  A bad
 * row (a count outside 0..u_cap, an id outside the vocabulary or the blank) is NaN / -1 as above, the call returns RS_EINVAL after
 * the sync and the other rows keep their bits.
 * Workspace: rs_rnnt_align_rows_workspace_bytes(ctx, B, R, tp_max, u_cap) is the MINIMUM, sized without sharing (what a group shares
 * is unknown before the ids are read): R x tp_max x (u_cap + 1) cells, 32 lattice rows per chunk; 0 for invalid arguments.
 * RS_EINVAL before anything is enqueued as for rs_rnnt_align (R in the place of B in the bound).  row_utt is checked on the device
 * before anything indexes with it: an entry below -1 or >= B, a decrease, or more than RS_ALIGN_ROWS_PER_UTT_MAX rows on one
 * utterance make the call return RS_EINVAL after the sync with NOTHING scored and no output written. */
enum { RS_ALIGN_NO_SHARING = 2 };
#define RS_ALIGN_ROWS_PER_UTT_MAX 64
size_t rs_rnnt_align_rows_workspace_bytes(const rs_ctx* ctx, int B, int R, int tp_max, int u_cap);
int rs_rnnt_align_rows(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt, int R,
                       const int32_t* ids, const int32_t* n_ids, int u_cap, int flags, float* loglik, float* best, int32_t* frames,
                       float* logp, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream);

/* rs_rnnt_token_scores over R rows with the same row_utt contract (a -1 row has no tokens: none of its slots is touched; a row_utt
 * error returns RS_EINVAL after the first sync with nothing scored).  ids / frames / logp / top1 [R][u_cap] and n_ids [R] are per
 * row; a frame is checked against the row's utterance.  The results equal rs_rnnt_token_scores on replicated frames, bit for bit.
 * Nothing is shared here: a text has only U joint rows.  Workspace: the minimum for R rows. */
size_t rs_rnnt_token_scores_rows_workspace_bytes(const rs_ctx* ctx, int B, int R, int u_cap);
int rs_rnnt_token_scores_rows(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt,
                              int R, const int32_t* ids, const int32_t* frames, const int32_t* n_ids, int u_cap, int flags, float* logp,
                              int32_t* top1, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC segmentation of a batch (ESPnet family: time stamps of a recognised text) ------------------
 * Replaces: ctc_segmentation.ctc_segmentation(config, lpz, ground_truth_mat) of the third-party aligner the reference calls
 * once per window (pkg/espnet-asr/src/ctc.py:60-75), for the default CtcSegmentationParameters — the only ones the reference
 * sets: blank_transition_cost_zero = False, preamble_transition_cost_zero = True, backtrack_from_max_t = False, max_prob = -1e10.
 *   probs f32[B*tp_max][ld]     the posteriors rs_encoder_set_ctc_out registered (row pitch ld >= vocabulary; columns past the
 *                               vocabulary and rows past enc_lens[b] are never read)
 *   enc_lens i32[B]             frames T of each utterance
 *   gt i32[B][c_max][S]         prepare_text's ground-truth matrix per utterance: the token that ENDS at symbol c and is s + 1
 *                               characters long, -1 = none (also the padding rows); gt_lens i32[B] = symbols C of each row
 *   blank                       column of the blank posterior
 *   frames i32[B][c_max]        the frame at which each symbol's switch transition was taken; 0 where the host aligner leaves its
 *                               `timings` at 0 (timings = frames * index_duration, in float64 on the host)
 *   status i32[B]               0 aligned; 1 more symbols than frames (the aligner's "Audio is shorter than text!"); 2 the
 *                               backtracking reached frame 0 before symbol 0 (the aligner's IndexError); 3 not alignable here: more
 *                               than 8000 frames (min_window_size; the aligner's own windowing is not restated), or lengths
 *                               outside tp_max / c_max
 * The forward table is float32 with adds and maxima only, in the aligner's order, and the backtracking comparisons are made in
 * double: frames equal the host aligner's to the last bit (csrc/k_ctc_align.hip).  Asynchronous on `stream`; no host round trip.
 * Workspace: rs_ctc_align_workspace_bytes (one decision byte per (b, t, c); 0 for invalid arguments), separate from
 * rs_workspace_bytes.  RS_EINVAL — before anything is enqueued — for S outside 1..8, c_max < 2, a blank outside the row pitch or
 * a workspace that is too small. */
size_t rs_ctc_align_workspace_bytes(const rs_ctx* ctx, int B, int tp_max, int c_max, int S);
int rs_ctc_align(rs_ctx* ctx, const float* probs, int ld, const int32_t* enc_lens, int B, int tp_max, const int32_t* gt,
                 const int32_t* gt_lens, int c_max, int S, int blank, int32_t* frames, int32_t* status, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- where to cut a long recording, for a batch of windows (ESPnet family) ---------------------------
 * Replaces: find_blank(model, samples, threshold) of the reference (pkg/espnet-asr/src/ctc.py:29-58), which scans the blank
 * posteriors of one 20 s window on the host, for B windows at once and without the column leaving the device.
 *   blank_prob f32[B*tp_max]    the blank column rs_encoder_set_ctc_out(ctx, NULL, col) registered: row b at b*tp_max with
 *                               enc_lens[b] valid frames; cells past enc_lens[b] are never read
 *   enc_lens i32[B]             frames T of each window
 *   n_samples i32[B]            samples n of each window (what the reference's len(samples) is)
 *   threshold                   a frame is silent when its blank posterior is > threshold, compared in float32
 *   cuts i32[B][2]              (start, end) in samples of the longest silent stretch: a maximal run of silent frames
 *                               [first, after) that a non-silent frame closes (after < T; a run that reaches the last frame is
 *                               ignored), mapped to samples as (int64)((double)idx / (double)(T + 1) * (double)n) — one double
 *                               division, one double multiplication, truncation, like Python's int(idx / (frames + 1) * n) —
 *                               and dropped when its start sample is 0.  The first stretch of the greatest end - start wins if
 *                               that length is > 0; otherwise, and for T == 0, the result is (n, n).  A row whose enc_lens[b]
 *                               lies outside 0..tp_max is written (-1, -1) and nothing of it is read.
 * One wavefront per window, 64 frames per step (csrc/k_ctc_blank.hip).  No workspace; asynchronous on `stream`; no host round
 * trip.  RS_EINVAL — before anything is enqueued — for a null context or pointer, B <= 0, tp_max <= 0 or a context of the
 * Zipformer / avsr families (they have no CTC head). */
int rs_ctc_find_blank(rs_ctx* ctx, const float* blank_prob, const int32_t* enc_lens, const int32_t* n_samples,
                      int B, int tp_max, float threshold, int32_t* cuts /* [B][2] */, void* stream);

/* ---- resample and down-mix a batch to the model's rate (added within ABI 7) ------------------------
 * Replaces: norm_audio of the reference (pkg/nemo-asr/src/audio.py:54-68; the espnet and k2 packages have the same function):
 * librosa.resample to 16 kHz, then librosa.to_mono — for a batch of recordings of ONE (rate, channel count), in one launch.
 * The filter is the caller's: a linear-phase low-pass h of `numtaps` (odd) taps at the internal rate orig * up = target * down,
 * up / down the reduced ratio (reazonspeech_amd/runtime/resample.py: plan(), the Kaiser-windowed sinc of the host path).
 *   x        f32: the rows' [channels][row_len[b]] planes back to back; row b begins at x + row_off[b] (floats)
 *   row_off  i64[B], row_len i32[B] (samples per channel)
 *   table    f32[up][Jp], Jp = ceil(numtaps / up) rounded up to a multiple of 4: table[p][j] = up * h[p + j * up], 0 beyond numtaps
 *   out      f32[B][out_pitch]: out[b][out_offset + n] = y[n] for n < n_out = ceil(row_len[b] * up / down),
 *              y[n] = sum over m of xm[m] * table-entry(half + n * down - m * up),  half = (numtaps - 1) / 2,
 *            where xm is the mean of the channels (sum in channel order, one division) and 0 outside the row — scipy's
 *            resample_poly cut to librosa's length, up to float32 rounding: one fmaf per tap in increasing j = q - m,
 *            q = (half + n * down) div up.  Every other element of the row, in front of out_offset and from out_offset + n_out
 *            to out_pitch, is written 0: the layout rs_frontend_logmel reads (audio_stride = out_pitch).  Outputs that would
 *            fall beyond out_pitch are not written.
 *   out_lens i32[B] = n_out
 * up = down = 1 with numtaps = 1 and table = {1, 0, 0, 0} is the down-mix alone.  A row's bits do not depend on the other rows of
 * the launch.  No workspace; asynchronous on `stream`; no host round trip (csrc/k_resample.hip).  RS_EINVAL — before anything is
 * enqueued — for a null context or pointer, B < 0, channels < 1, up / down / numtaps outside 1..2^24, an even numtaps, an
 * out_offset outside 0..out_pitch, or a ratio whose window of 255 * down / up + 2 + Jp samples exceeds 16384 (the caller
 * resamples such a rate on the host). */
int rs_resample(rs_ctx* ctx, const float* x, const int64_t* row_off, const int32_t* row_len, int B, int channels, const float* table,
                int up, int down, int numtaps, float* out, int64_t out_pitch, int out_offset, int32_t* out_lens, void* stream);

/* ---- AV-HuBERT feature extraction: raw audio and mouth crops in (added within ABI 7) ------------------
 * Replaces: AVHubertFeatureExtractor.__call__ of the reference (pkg/avsr/src/avhubert/feature_extraction_avhubert.py:120-158,
 * :199-232; reazonspeech_amd/avsr/feature_extraction.py is the host path these are pinned to) for decoded input: 16 kHz float32
 * samples and uint8 mouth crops.  The extractor exists without a model, so both take a device index and a stream instead of a
 * context (like rs_stream_create); the tables are the caller's (reazonspeech_amd/runtime/avsr_features.py: plan()).  No workspace;
 * asynchronous on `stream`; no host round trip (csrc/k_avsr_features.hip).  They return RS_EINVAL — before anything is enqueued —
 * for the arguments listed below, RS_EHIP when the device cannot be selected or a launch is refused, and set no error text.
 *
 * rs_avsr_logfbank: one launch per batch, python_speech_features.logfbank with its defaults + the 4-frame stacker + F.layer_norm.
 *   audio    f32: the clips back to back; clip b is audio[row_off[b] .. row_off[b] + row_len[b])
 *   row_off  i64[B] (floats), row_len i32[B] (samples; < 0: a clip without audio — its rows are zeros)
 *   twiddle  f32[256][2] = (cos, -sin)(2 pi j / 512), 8-byte aligned
 *   fb_idx   i32[26][2] = (first bin, tap count <= RS_AVSR_FBANK_MAXW) of each triangular filter,
 *   fb_w     f32[26][RS_AVSR_FBANK_MAXW] its taps: the mel filterbank of logfbank, banded
 *   out      f32[B][T][26 * stack]:
 *     s'[0] = s[0], s'[i] = s[i] - 0.97 s[i-1] over the whole clip;  frame f = s'[160 f .. 160 f + 400), 0 beyond the clip;
 *     frames = 1 if n <= 400 else 1 + ceil((n - 400) / 160);
 *     E[f][m] = sum_k fb[m][k] * |DFT512(frame f)[k]|^2 / 512 over the bins k = 0 .. 256;
 *     L[f][m] = logf(E[f][m] == 0 ? 2.220446e-16 : E[f][m])           (float64 machine epsilon; the accurate logf)
 *     row r = L[stack r .. stack r + stack) flattened, frames >= `frames` as zeros (not log(eps)); rows >= ceil(frames / stack)
 *     are all zero;  normalize != 0: (x - mean) / sqrt(var + 1e-5) over the 26 * stack features of every row < T, two-pass,
 *     biased variance, no affine (a zero row stays exactly 0).
 *   All of it in float32 (the host path evaluates logfbank in float64).  A row's bits do not depend on the other rows of the launch.
 *   RS_EINVAL: a null pointer (B > 0), B < 0, T < 1, stack outside 1..8, a misaligned twiddle table.
 *
 * rs_avsr_pixels: one launch per group of clips whose frames share (H, W, channels).
 *   frames     u8 [n_frames][H][W] grey or [n_frames][H][W][3] BGR, the group's clips back to back, 4-byte aligned
 *   frame_idx  i32[B][idx_pitch]: the source frame of output frame (b, t < T) — the nearest-frame alignment to the audio rate is
 *              the caller's; -1 (or an index >= n_frames) = a padding frame or a clip without video: grey level 0; < -1 = the
 *              output frame belongs to another launch and is not written
 *   lut        f32[256]: the value of each grey level, (float32(u) / 255 - mean) / std as the host path rounds it
 *   out        f32[B][T][crop][crop], 16-byte aligned:
 *     out[b][t][y][x] = lut[grey(frames[frame_idx[b][t]][top + y][left + x])],
 *     grey(B, G, R) = (1868 B + 9617 G + 4899 R + 8192) >> 14 in integers (OpenCV's 8-bit COLOR_BGR2GRAY) for channels == 3.
 *   RS_EINVAL: a null pointer (B > 0), B < 0, T < 1, n_frames < 0, H / W < 1, crop no positive multiple of 4 (the model takes
 *   multiples of 8), a crop window outside the frame
 *   (top < 0, left < 0, top + crop > H, left + crop > W), channels not 1 or 3, idx_pitch < T, misaligned frames / out. */
#define RS_AVSR_FBANK_FILTERS 26
#define RS_AVSR_FBANK_MAXW 48
int rs_avsr_logfbank(int device, const float* audio, const int64_t* row_off, const int32_t* row_len, int B, int T, int stack,
                     int normalize, const float* twiddle, const int32_t* fb_idx, const float* fb_w, float* out, void* stream);
int rs_avsr_pixels(int device, const uint8_t* frames, int64_t n_frames, int H, int W, int channels, const int32_t* frame_idx,
                   int idx_pitch, int B, int T, int crop, int top, int left, const float* lut, float* out, void* stream);

/* ---- profiling hooks for bench.py (roofline.achieved) ------------------------------------
 * When enabled, the launcher brackets every launch of the selected kernel class with HIP
 * events on the launch stream.  rs_profile_read synchronises those events and returns the
 * accumulated milliseconds, launch count and algorithmic FLOPs / bytes since the last reset. */
enum { RS_PROF_NONE = 0, RS_PROF_GEMM = 1, RS_PROF_ATTN = 2, RS_PROF_FRONTEND = 4,
       RS_PROF_DECODE = 8, RS_PROF_ELEMENTWISE = 16, RS_PROF_SUBSAMPLE = 32 };
int rs_profile_enable(rs_ctx* ctx, int class_mask);
int rs_profile_read(rs_ctx* ctx, int klass, double* ms, int64_t* launches, double* flops,
                    double* bytes);
int rs_profile_reset(rs_ctx* ctx);
/* Per-launch detail of a class since the last reset, in launch order: shapes[4 * i ..] = (M, N, K, flags) for GEMM launches
 * (zeros for other classes), flops[i], ms[i].  Up to `cap` records are copied (arrays may be NULL); *n_out = how many exist.
 * bench.py groups them into `roofline.per_shape`. */
int rs_profile_read_launches(rs_ctx* ctx, int klass, int32_t* shapes, double* flops, float* ms, int cap, int* n_out);

/* ---- single-operator entry points (parity tests call these one by one) -------------------*/

/* C[M][N] = epilogue(A[M][K] . W[N][K]^T); A, W bf16 row-major, K % 64 == 0; bf16 output needs N % 8 == 0, f32 N % 4 == 0.
 * flags: see RS_GEMM_* ; bias f32[N]; residual f32[M][ldc] (may alias out when out is f32); RS_GEMM_ROWMASK combines
 * with bf16 output only.  One kernel family serves every shape and an output row's bits do not depend on M or on the
 * tile height the launcher picks (batch invariance of the encoder). */
enum { RS_GEMM_BIAS = 1, RS_GEMM_RELU = 2, RS_GEMM_SILU = 4, RS_GEMM_RESIDUAL = 8,
       RS_GEMM_OUT_F32 = 16, RS_GEMM_ROWMASK = 32,
       /* out bf16[M][N/2] = (a + bias_a) * sigmoid(g + bias_g): columns 64j .. 64j+31 of the product are values,
        * 64j+32 .. 64j+63 their gates (weight rows interleaved in blocks of 32, see rs_set_tensor); bias only,
        * N % 64 == 0 */
       RS_GEMM_GLU = 64,
       /* icefall's SwooshL / SwooshR activations (the Zipformer family; plain bf16 or f32 output only) */
       RS_GEMM_SWOOSHL = 128, RS_GEMM_SWOOSHR = 256,
       /* exact GELU, 0.5 x (1 + erf(x / sqrt 2)) (the AV-HuBERT family; rs_gemm_f32 only) */
       RS_GEMM_GELU = 512 };
int rs_gemm_bf16(rs_ctx* ctx, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                 void* out, int ldc, int M, int N, int K, int flags, const float* bias, float alpha,
                 const float* residual, const int32_t* mask_lens, int mask_rows_per_step,
                 int mask_steps, void* stream);

/* The float32 parity mode's operators (rs_set_option "precision_f32"), one by one: the same contracts as rs_gemm_bf16 (flags
 * BIAS / RELU / SILU / RESIDUAL / ROWMASK; K % 32 == 0, N % 4 == 0), rs_relpos_attention (any head_dim <= 256) and
 * rs_glu_dwconv_silu (x f32[B*T][2*d], values | gates) on float32 tensors. */
int rs_gemm_f32(rs_ctx* ctx, const float* A, int lda, const float* W, int ldw, float* out, int ldc, int M, int N, int K,
                int flags, const float* bias, float alpha, const float* residual, const int32_t* mask_lens,
                int mask_rows_per_step, int mask_steps, void* stream);
int rs_relpos_attention_f32(rs_ctx* ctx, const float* qkv, const float* pos, const float* bias_u, const float* bias_v,
                            const int32_t* lens, int B, int T, float* ctx_out, void* stream);
/* The int8 mode's operator (rs_set_option "precision_i8"): onnxruntime's dynamically quantized MatMul
 * (DynamicQuantizeLinear -> MatMulInteger -> Cast -> Mul(sx * sw) -> bias Add), restated per GROUP of `group` rows (one group per
 * utterance, M = n_groups * group).  For group g: sx = (max(0, max x) - min(0, min x)) / 255 (1 when that is 0) and
 * zx = round(-min(0, min x) / sx) over the first lens[g] rows of A (columns < K), written to qp f32 [n_groups][2] = (sx, zx);
 * xq = clamp(round(x / sx) + zx, 0, 255) (round half to even, x / sx correctly rounded);
 * out[m][n] = epilogue(float(sum_{k < K} (xq[m][k] - zx) (W[n][k] - zw)) * fl(sx * sw) + bias[n]), the integer sum exact
 * (v_mfma_i32_16x16x64_i8), then SWOOSHL or SWOOSHR, then + residual[m][n] (pitch ldc, may alias out).
 * A f32 [M][lda]; W int8 [N][ldw] (ldw % 16 == 0, 16-byte aligned, columns >= K ignored); colsum int32 [N] = sum_{k < K} W[n][k];
 * wq f32 [2] = (sw, zw) on the device; flags: RS_GEMM_BIAS / SWOOSHL / SWOOSHR / RESIDUAL (RS_GEMM_OUT_F32 implied). */
int rs_gemm_i8q(rs_ctx* ctx, const float* A, int lda, const int32_t* lens, int group, const int8_t* W, int ldw, const int32_t* colsum,
                const float* wq, float* out, int ldc, int M, int N, int K, int flags, const float* bias, const float* residual, float* qp,
                void* stream);
int rs_glu_dwconv_silu_f32(rs_ctx* ctx, const float* x, const float* dw_w, const float* dw_b, const int32_t* lens, int B,
                           int T, int d, int k, float* out, void* stream);

/* y = LayerNorm(x) over the last dim (d); x f32[M][d]; out_bf16 and/or out_f32 may be NULL. */
int rs_layernorm(rs_ctx* ctx, const float* x, const float* gamma, const float* beta, int M, int d,
                 float eps, uint16_t* out_bf16, float* out_f32, void* stream);

/* Relative-position multi-head attention core.
 *   qkv bf16[B*T][3*d_model] (q | k | v), pos bf16[2T-1][d_model] (linear_pos of the table),
 *   bias_u/bias_v f32[n_heads][128], lens i32[B]; ctx_out bf16[B*T][d_model]. */
int rs_relpos_attention(rs_ctx* ctx, const uint16_t* qkv, const uint16_t* pos, const float* bias_u,
                        const float* bias_v, const int32_t* lens, int B, int T, uint16_t* ctx_out,
                        void* stream);

/* Conv-module middle: GLU -> zero padded frames -> depthwise k (BatchNorm folded) -> SiLU.
 *   x bf16[B*T][2*d], dw_w f32[k][d] (tap-major), dw_b f32[d]; out bf16[B*T][d]. */
int rs_glu_dwconv_silu(rs_ctx* ctx, const uint16_t* x, const float* dw_w, const float* dw_b,
                       const int32_t* lens, int B, int T, int d, int k, uint16_t* out, void* stream);
/* The same operator for the other layouts of its input: RS_GLU_HALVES = the layout above (values | gates);
 * RS_GLU_BLOCK32 = x bf16[B*T][2*d] with values / gates interleaved in blocks of 32 columns (the plain product of
 * the interleaved pw1 weight); RS_GLU_APPLIED = x bf16[B*T][d], GLU already applied by RS_GEMM_GLU. */
enum { RS_GLU_HALVES = 0, RS_GLU_BLOCK32 = 1, RS_GLU_APPLIED = 2 };
int rs_glu_dwconv_silu_layout(rs_ctx* ctx, const uint16_t* x, int layout, const float* dw_w, const float* dw_b,
                              const int32_t* lens, int B, int T, int d, int k, uint16_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RS_ASR_H */
