// rs_api.hip — the C ABI of librs_asr.so (include/rs_asr.h): context lifecycle, weight registry, the family guard (rs_family.h) at
// every entry and the dispatch to the family that serves it, argument checks, profiling readers and the single-operator hooks.
// The families' own finalize, workspace plans and encoder call sequences live in k_conformer.hip, k_zipformer.hip and k_avsr.hip.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <set>
#include <utility>

#include "rs_common.h"
#include "rs_ngram_check.h"

size_t rs_rnnt_workspace_bytes(const rs_ctx* ctx, int B);
size_t rs_rnnt_alsd_workspace_bytes_impl(const rs_ctx* ctx, int B, int beam, int cap, bool hotwords, bool lm, int nbest);
size_t rs_rnnt_mbs_workspace_bytes_impl(const rs_ctx* ctx, int B, int K, int tp_max, bool hotwords, bool lm);
int rs_rnnt_mbs_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int K, float blank_penalty,
                     int length_norm, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int nbest, float* norm_scores,
                     int32_t* n_hyps, const rs_hotwords* hotwords, const int32_t* graph_of, const rs_ngram* ngram, float lm_alpha,
                     void* workspace, size_t workspace_bytes, hipStream_t s);
size_t rs_rnnt_beam_workspace_bytes_impl(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, bool hotwords, bool lm);
int rs_rnnt_beam_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int score_norm,
                      int max_pops, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int32_t* pops, int nbest,
                      float* norm_scores, int32_t* n_hyps, const rs_hotwords* hotwords, const int32_t* graph_of, const rs_ngram* ngram,
                      float lm_alpha, void* workspace, size_t workspace_bytes, hipStream_t s);
int rs_rnnt_alsd_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, double ratio,
                      int abs_len, int score_norm, int merge, int out_cap, int32_t* ids, int32_t* steps, int32_t* n_ids,
                      float* scores, int nbest, float* norm_scores, int32_t* n_hyps, const rs_hotwords* hotwords, const int32_t* graph_of, const rs_ngram* ngram, float lm_alpha,
                      void* workspace, size_t workspace_bytes, hipStream_t s);
size_t rs_rnnt_token_scores_workspace_bytes_impl(const rs_ctx* ctx, int B, int u_cap);
size_t rs_rnnt_align_workspace_bytes_impl(const rs_ctx* ctx, int B, int tp_max, int u_cap);
int rs_rnnt_align_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                       const int32_t* n_ids, int u_cap, int one_per_frame, float* loglik, float* best, int32_t* frames, float* logp,
                       void* workspace, size_t workspace_bytes, hipStream_t s);
int rs_rnnt_token_scores_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                              const int32_t* frames, const int32_t* n_ids, int u_cap, int steps, float* logp, int32_t* top1,
                              void* workspace, size_t workspace_bytes, hipStream_t s);
size_t rs_rnnt_align_rows_workspace_bytes_impl(const rs_ctx* ctx, int R, int tp_max, int u_cap);
int rs_rnnt_align_rows_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt,
                            int R, const int32_t* ids, const int32_t* n_ids, int u_cap, int one_per_frame, int no_sharing,
                            float* loglik, float* best, int32_t* frames, float* logp, int64_t* stats, void* workspace,
                            size_t workspace_bytes, hipStream_t s);
int rs_rnnt_token_scores_rows_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max,
                                   const int32_t* row_utt, int R, const int32_t* ids, const int32_t* frames, const int32_t* n_ids,
                                   int u_cap, int steps, float* logp, int32_t* top1, void* workspace, size_t workspace_bytes,
                                   hipStream_t s);
size_t rs_ctc_align_workspace_bytes_impl(int B, int tp_max, int c_max);
int rs_ctc_align_impl(rs_ctx* ctx, const float* probs, int ld, const int32_t* enc_lens, int B, int tp_max, const int32_t* gt,
                      const int32_t* gt_lens, int c_max, int S, int blank, int32_t* frames, int32_t* status, void* ws, hipStream_t s);
int rs_ctc_find_blank_impl(rs_ctx* ctx, const float* blank_prob, const int32_t* enc_lens, const int32_t* n_samples, int B, int tp_max,
                           float threshold, int32_t* cuts, hipStream_t s);
int rs_resample_impl(rs_ctx* ctx, const float* x, const int64_t* row_off, const int32_t* row_len, int B, int channels, const float* table,
                     int up, int down, int numtaps, float* out, long long out_pitch, int out_offset, int32_t* out_lens, hipStream_t s);
hipError_t rs_avsr_logfbank_launch(const float* audio, const int64_t* row_off, const int32_t* row_len, int B, int T, int stack, int normalize,
                                   const float* twiddle, const int32_t* fb_idx, const float* fb_w, float* out, hipStream_t s);
hipError_t rs_avsr_pixels_launch(const uint8_t* frames, long long n_frames, int H, int W, int channels, const int32_t* frame_idx, int idx_pitch,
                                 int B, int T, int crop, int top, int left, const float* lut, float* out, hipStream_t s);
int rs_rnnt_greedy_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int u_max,
                        int32_t* ids, int32_t* frames, int32_t* n_ids, void* workspace, size_t workspace_bytes,
                        hipStream_t s);

int rs_fail(rs_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int rs_n_cus(rs_ctx* ctx) {
    if (ctx->n_cus <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->n_cus = n;
    }
    return ctx->n_cus;
}

// test and A/B hooks over the table of rs_knobs.h, by environment name (deliberately not in rs_asr.h, like rs_debug_conv3x3_f32)
extern "C" int rs_debug_set_knob(const char* env_name, int value) { return rs_knob_set_named(env_name, value); }
extern "C" int rs_debug_get_knob(const char* env_name, int* value) { return rs_knob_get_named(env_name, value); }

int rs_ensure_dynamic_lds(rs_ctx* ctx, const void* func, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(ctx->device, func);
    if (done.count(key)) return RS_OK;
    // the attribute applies to the calling thread's CURRENT device: set it on the context's device whatever is current
    // (a caller may drive two GPUs from one thread), and leave the caller's current device as it was
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return rs_fail(ctx, RS_EHIP, "hipGetDevice failed");
    if (cur != ctx->device && hipSetDevice(ctx->device) != hipSuccess)
        return rs_fail(ctx, RS_EHIP, "hipSetDevice(%d) failed", ctx->device);
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (cur != ctx->device) hipSetDevice(cur);
    if (e != hipSuccess) return rs_fail(ctx, RS_EHIP, "cannot reserve %d bytes of dynamic LDS on device %d", bytes, ctx->device);
    done.insert(key);
    return RS_OK;
}

// ---- profiling ---------------------------------------------------------------------------------
int rs_prof_class_index(int klass) {
    int i = 0;
    while (klass > 1) { klass >>= 1; ++i; }
    return i;
}
void rs_prof_begin(rs_ctx* ctx, int klass, hipStream_t s, double flops, double bytes) {
    if (!(ctx->prof_mask & klass)) return;
    rs_prof_slot& p = ctx->prof[rs_prof_class_index(klass)];
    if (p.used + 2 > p.ev.size()) {
        const size_t old = p.ev.size();
        p.ev.resize(old + 512);
        for (size_t i = old; i < p.ev.size(); ++i) hipEventCreate(&p.ev[i]);
    }
    hipEventRecord(p.ev[p.used], s);
    p.flops += flops;
    p.bytes += bytes;
    p.launches += 1;
    if (p.detail.size() < (1u << 20)) p.detail.push_back(rs_prof_launch{ctx->prof_tag[0], ctx->prof_tag[1], ctx->prof_tag[2], ctx->prof_tag[3], flops, -1.0f});
    ctx->prof_tag[0] = ctx->prof_tag[1] = ctx->prof_tag[2] = ctx->prof_tag[3] = 0;
}
void rs_prof_end(rs_ctx* ctx, int klass, hipStream_t s) {
    if (!(ctx->prof_mask & klass)) return;
    rs_prof_slot& p = ctx->prof[rs_prof_class_index(klass)];
    hipEventRecord(p.ev[p.used + 1], s);
    p.used += 2;
}

extern "C" {

int rs_abi_version(void) { return RS_ABI_VERSION; }

void rs_destroy(rs_ctx* ctx) {
    RS_GUARD_QUERY(ctx, rs_destroy, );
    for (auto& p : ctx->prof)
        for (auto e : p.ev) hipEventDestroy(e);
    for (auto& kv : ctx->wfm) (void)hipFree(kv.second);
    if (ctx->wfm_scratch) (void)hipFree(ctx->wfm_scratch);
    delete ctx;
}

const char* rs_last_error(const rs_ctx* ctx) {
    RS_GUARD_QUERY(ctx, rs_last_error, "null context");
    return ctx->err.c_str();
}

int rs_set_tensor(rs_ctx* ctx, const char* name, const void* dev_ptr, size_t nbytes) {
    RS_GUARD(ctx, rs_set_tensor);
    if (!name || !dev_ptr) return RS_EINVAL;
    ctx->tensors[name] = {dev_ptr, nbytes};
    ctx->finalized = false;
    return RS_OK;
}

}  // extern "C"

void rs_get_screened_joint(rs_ctx* ctx, rs_weights& r) {
    const size_t V = ctx->d.n_logits, J = ctx->d.joint_hidden, Vpad = (V + 15) / 16 * 16;
    ctx->jout_w16 = nullptr; ctx->jout_wrm = ctx->jout_bpad = ctx->jout_wmax = nullptr;
    if (!r.has("joint.out.w16") && !r.has("joint.out.wrm") && !r.has("joint.out.bpad") && !r.has("joint.out.wmax")) return;
    r.get("joint.out.w16", Vpad * J, ctx->jout_w16);
    r.get("joint.out.wrm", V * J, ctx->jout_wrm);
    r.get("joint.out.bpad", Vpad, ctx->jout_bpad);
    r.get("joint.out.wmax", 4, ctx->jout_wmax);
}

extern "C" {

int rs_finalize(rs_ctx* ctx) {
    RS_GUARD(ctx, rs_finalize);
    switch (ctx->family) {
        case RS_FAM_ZIPFORMER: return rs_k2_finalize_impl(ctx);
        case RS_FAM_AVSR: return rs_avsr_finalize_impl(ctx);
        default: return rs_conformer_finalize_impl(ctx);
    }
}

int rs_stream_create(void** out, int device, const uint32_t* cu_mask, int n_words, int priority) {
    if (!out) return RS_EINVAL;
    *out = nullptr;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return RS_EHIP;
    if (cur != device && hipSetDevice(device) != hipSuccess) return RS_EHIP;
    hipStream_t s = nullptr;
    hipError_t e;
    if (cu_mask && n_words > 0) e = hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, cu_mask);
    else e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (cur != device) hipSetDevice(cur);          // the caller's current device is not a side effect of this call
    if (e != hipSuccess) return RS_EHIP;
    *out = (void*)s;
    return RS_OK;
}

int rs_stream_destroy(void* stream) {
    if (!stream) return RS_OK;
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? RS_OK : RS_EHIP;
}

}  // extern "C"

namespace {

// rs_set_option: one row per key.  A setter returns RS_OK or refuses the value with its own text.
struct rs_option_row { const char* key; int serves; int (*set)(rs_ctx* ctx, int value); };
const rs_option_row rs_option_rows[] = {
    {"decode_screen", RS_SERVES_CZ, [](rs_ctx* ctx, int v) { ctx->decode_screen = v != 0; return (int)RS_OK; }},
    {"decode_narrow", RS_SERVES_CZ, [](rs_ctx* ctx, int v) { ctx->decode_narrow = v != 0; return (int)RS_OK; }},
    {"precision_f32", RS_SERVES_CZ, [](rs_ctx* ctx, int v) {
         if (v && !ctx->has_f32)
             return rs_fail(ctx, RS_EMISSING, "precision_f32: the float32 weights (\"*.f32\" tensors) are not registered / rs_finalize has not run");
         ctx->precision_f32 = v != 0;
         return (int)RS_OK;
     }},
    // the float32 encoder with its quantized Linears ("*.i8") as onnxruntime's int8 MatMul
    {"precision_i8", RS_SERVES_Z, [](rs_ctx* ctx, int v) {
         if (v && !(ctx->has_f32 && ctx->has_i8))
             return rs_fail(ctx, RS_EMISSING, "precision_i8: the float32 weights (\"*.f32\") and the quantized ones (\"*.i8\") must be registered and rs_finalize run");
         ctx->precision_i8 = v != 0;
         return (int)RS_OK;
     }},
    // float32 products as three bf16 matrix-core terms (k_f32.hip X3): the AV-HuBERT family, and the "precision_f32" mode of the
    // others ("fp32x3": not an IEEE chain; held to the same goldens)
    {"gemm_f32_x3", RS_SERVES_ALL, [](rs_ctx* ctx, int v) { ctx->gemm_f32_x3 = v != 0; return (int)RS_OK; }},
    // conv2 with its patches gathered into LDS (1, default) or as patch matrix + GEMM launch (0): same bits
    {"k2_conv2_fused", RS_SERVES_Z, [](rs_ctx* ctx, int v) { ctx->k2_conv2_fused = v != 0; return (int)RS_OK; }},
    // the ConvNeXt pointwise pair as one kernel (1, default) or as two GEMM launches (0): same bits
    {"k2_cnx_fused", RS_SERVES_Z, [](rs_ctx* ctx, int v) { ctx->k2_cnx_fused = v != 0; return (int)RS_OK; }},
    {"fuse_glu", RS_SERVES_C, [](rs_ctx* ctx, int v) {
         if (v < 0 || v > 1) return rs_fail(ctx, RS_EINVAL, "fuse_glu must be 0 or 1");
         rs_conformer_of(ctx)->fuse_glu = v;
         return (int)RS_OK;
     }},
    {"defer_out_norm", RS_SERVES_C, [](rs_ctx* ctx, int v) { rs_conformer_of(ctx)->defer_out_norm = v != 0; return (int)RS_OK; }},
};

}  // namespace

extern "C" {

int rs_set_option(rs_ctx* ctx, const char* key, int value) {
    RS_GUARD(ctx, rs_set_option);
    if (!key) return RS_EINVAL;
    for (const rs_option_row& row : rs_option_rows) {
        if (strcmp(key, row.key)) continue;
        if (row.serves & (1 << ctx->family)) return row.set(ctx, value);
        return rs_fail(ctx, RS_EINVAL, "rs_set_option: option '%s' does not apply to %s context%s", key, rs_family_name(ctx->family),
                       row.serves == RS_SERVES_Z ? " (it applies to a Zipformer context only)" : "");
    }
    return rs_fail(ctx, RS_EINVAL, "unknown option '%s'", key);
}

int rs_encoder_set_taps(rs_ctx* ctx, float* sub_out, float* layer_out, const int32_t* layer_ids, int n_layer_ids) {
    RS_GUARD(ctx, rs_encoder_set_taps);
    if (n_layer_ids < 0 || (n_layer_ids > 0 && (!layer_out || !layer_ids))) return rs_fail(ctx, RS_EINVAL, "taps: null pointer");
    for (int i = 0; i < n_layer_ids; ++i)
        if (layer_ids[i] < 0 || layer_ids[i] >= ctx->d.n_layers) return rs_fail(ctx, RS_EINVAL, "taps: layer %d out of range", layer_ids[i]);
    rs_conformer& cf = *rs_conformer_of(ctx);
    cf.tap_sub = sub_out;
    cf.tap_layers = n_layer_ids > 0 ? layer_out : nullptr;
    cf.tap_ids.assign(layer_ids, layer_ids + n_layer_ids);
    return RS_OK;
}

int rs_mel_frames(const rs_ctx* ctx, int n_samples) {
    RS_GUARD_QUERY(ctx, rs_mel_frames, 0);
    const rs_dims& d = ctx->d;
    if (d.hop_length <= 0) return 0;
    if (d.frontend_kind == 2) return (n_samples + d.hop_length / 2) / d.hop_length;     // kaldi, snip_edges = false
    return n_samples / d.hop_length + (d.frontend_kind == 1 ? 1 : 0);
}

int rs_enc_frames(const rs_ctx* ctx, int n) {
    RS_GUARD_QUERY(ctx, rs_enc_frames, 0);
    if (ctx->family == RS_FAM_ZIPFORMER) return rs_k2_enc_frames_impl(ctx, n);
    for (int s = 0; s < ctx->d.sub_stages; ++s) n = rs_conv_len(n, ctx->d.sub_kind);
    return n;
}

int rs_encoder_set_ctc_out(rs_ctx* ctx, float* probs, float* blank_prob) {
    RS_GUARD(ctx, rs_encoder_set_ctc_out);
    if ((probs || blank_prob) && ctx->d.ctc_vocab <= 0) return rs_fail(ctx, RS_EINVAL, "this model has no CTC head (rs_dims.ctc_vocab)");
    rs_conformer_of(ctx)->ctc_probs = probs;
    rs_conformer_of(ctx)->ctc_blank = blank_prob;
    return RS_OK;
}

size_t rs_workspace_bytes(const rs_ctx* ctx, int B, int max_samples) {
    RS_GUARD_QUERY(ctx, rs_workspace_bytes, 0);
    if (B <= 0 || max_samples < 0) return 0;
    const int t_max = rs_mel_frames(ctx, max_samples);
    const size_t fe = rs_align((size_t)B * (t_max > 0 ? t_max : 1) * ctx->d.n_mels * 4) + 256;
    const size_t enc = ctx->family == RS_FAM_ZIPFORMER ? rs_k2_workspace_bytes_impl(ctx, B, t_max) : rs_conformer_workspace_bytes_impl(ctx, B, t_max);
    const size_t dec = rs_rnnt_workspace_bytes(ctx, B);
    const size_t m = fe > enc ? fe : enc;
    return m > dec ? m : dec;
}

int rs_host_stage_rows(float* dst, size_t dst_pitch, int width, const float* const* rows, const int32_t* lens,
                       int n_rows, int total_rows, int32_t* dst_lens) {
    if (!dst || !dst_lens || n_rows < 0 || total_rows < n_rows || width < 0 || (size_t)width > dst_pitch) return RS_EINVAL;
    if (n_rows > 0 && (!rows || !lens)) return RS_EINVAL;
    for (int b = 0; b < n_rows; ++b) {
        const int n = lens[b];
        if (n < 0 || n > width || (n > 0 && !rows[b])) return RS_EINVAL;
        float* row = dst + (size_t)b * dst_pitch;
        if (n > 0) memcpy(row, rows[b], (size_t)n * sizeof(float));
        if (n < width) memset(row + n, 0, (size_t)(width - n) * sizeof(float));
        dst_lens[b] = n;
    }
    for (int b = n_rows; b < total_rows; ++b) dst_lens[b] = 0;
    return RS_OK;
}

int rs_frontend_logmel(rs_ctx* ctx, const float* audio, const int32_t* lens, int B, int audio_stride,
                       int pad_left, int pad_right, int t_max, float* feats, int32_t* n_frames, void* workspace,
                       size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_frontend_logmel);
    if (B < 0 || t_max < 0 || pad_left < 0 || pad_right < 0) return rs_fail(ctx, RS_EINVAL, "frontend: negative size");
    if (B == 0 || t_max == 0) return RS_OK;
    if (!audio || !lens || !feats || !n_frames || !workspace) return rs_fail(ctx, RS_EINVAL, "frontend: null pointer");
    const size_t need = (size_t)B * t_max * ctx->d.n_mels * 4;
    if (workspace_bytes < need) return rs_fail(ctx, RS_EWORKSPACE, "frontend: workspace %zu < %zu", workspace_bytes, need);
    return rs_launch_frontend(ctx, audio, lens, B, audio_stride, pad_left, pad_right, t_max, feats, n_frames,
                              reinterpret_cast<float*>(workspace), (hipStream_t)stream);
}

int rs_encoder_forward(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max, float* enc_out,
                       float* joint_enc, int32_t* enc_lens, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_encoder_forward);
    if (B <= 0 || t_max <= 0) return B < 0 || t_max < 0 ? rs_fail(ctx, RS_EINVAL, "encoder: negative size") : RS_OK;
    if (!feats || !n_frames || !joint_enc || !enc_lens || !workspace) return rs_fail(ctx, RS_EINVAL, "encoder: null pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (ctx->family) {
        case RS_FAM_ZIPFORMER: return rs_k2_encoder_forward_impl(ctx, feats, n_frames, B, t_max, enc_out, joint_enc, enc_lens, workspace, workspace_bytes, s);
        default: return rs_conformer_encoder_forward_impl(ctx, feats, n_frames, B, t_max, enc_out, joint_enc, enc_lens, workspace, workspace_bytes, s);
    }
}

int rs_rnnt_greedy(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int u_max,
                   int32_t* ids, int32_t* frames, int32_t* n_ids, void* workspace, size_t workspace_bytes,
                   void* stream) {
    RS_GUARD(ctx, rs_rnnt_greedy);
    if (B < 0 || tp_max < 0 || u_max < 0) return rs_fail(ctx, RS_EINVAL, "rnnt: negative size");
    if (B == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !frames || !n_ids || !workspace) return rs_fail(ctx, RS_EINVAL, "rnnt: null pointer");
    if (tp_max == 0) { RS_HIP(ctx, hipMemsetAsync(n_ids, 0, (size_t)B * 4, (hipStream_t)stream)); return RS_OK; }
    return rs_rnnt_greedy_impl(ctx, joint_enc, enc_lens, B, tp_max, u_max, ids, frames, n_ids, workspace,
                               workspace_bytes, (hipStream_t)stream);
}

static int alsd_steps(int tp_max, double ratio, int abs_len) {
    const int budget = abs_len >= 0 ? abs_len : (int)(ratio * (double)tp_max);
    return tp_max + budget > 0 ? tp_max + budget : 1;
}

// the three workspace queries of ALSD (each entry keeps its own family guard): room for the hotword states and / or the LM states
static size_t alsd_workspace(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs, bool hotwords,
                             bool lm, int nbest = 0) {
    if (B <= 0 || beam <= 0 || tp_max < 0 || (max_target_abs < 0 && !(max_target_ratio >= 0.0))) return 0;
    const int W = beam < ctx->d.n_logits - 1 ? beam : ctx->d.n_logits - 1;
    return rs_rnnt_alsd_workspace_bytes_impl(ctx, B, W, alsd_steps(tp_max, max_target_ratio, max_target_abs), hotwords, lm, nbest);
}

size_t rs_rnnt_alsd_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs) {
    RS_GUARD_QUERY(ctx, rs_rnnt_alsd_workspace_bytes, 0);
    return alsd_workspace(ctx, B, beam, tp_max, max_target_ratio, max_target_abs, false, false);
}

size_t rs_rnnt_alsd_hotwords_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs) {
    RS_GUARD_QUERY(ctx, rs_rnnt_alsd_hotwords_workspace_bytes, 0);
    return alsd_workspace(ctx, B, beam, tp_max, max_target_ratio, max_target_abs, true, false);
}

size_t rs_rnnt_alsd_lm_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs) {
    RS_GUARD_QUERY(ctx, rs_rnnt_alsd_lm_workspace_bytes, 0);
    return alsd_workspace(ctx, B, beam, tp_max, max_target_ratio, max_target_abs, true, true);
}

// the argument checks and the dispatch of rs_rnnt_alsd, rs_rnnt_alsd_hotwords, rs_rnnt_alsd_lm (hw == nullptr, lm == nullptr: the
// plain kernels) and rs_rnnt_alsd_nbest (nbest >= 1: ids / steps [B][nbest][out_cap], n_ids / scores / norm_scores [B][nbest],
// n_hyps [B]; the others pass nbest = 0 and no lists: the one result)
static int alsd_call(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, double max_target_ratio,
                     int max_target_abs, int flags, int out_cap, int32_t* ids, int32_t* steps, int32_t* n_ids, float* scores, int nbest,
                     float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm, float lm_alpha, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (B < 0 || tp_max < 0 || out_cap < 0) return rs_fail(ctx, RS_EINVAL, "alsd: negative size");
    if (max_target_abs < 0 && !(max_target_ratio >= 0.0 && max_target_ratio <= 64.0))
        return rs_fail(ctx, RS_EINVAL, "alsd: max_target_ratio must be in [0, 64]");
    if (B == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !steps || !n_ids || !scores || !workspace) return rs_fail(ctx, RS_EINVAL, "alsd: null pointer");
    if (nbest > 0 && (!norm_scores || !n_hyps)) return rs_fail(ctx, RS_EINVAL, "alsd: null pointer");
    if (tp_max == 0) {                                    // no frames anywhere: the start hypothesis, empty, score 0
        const size_t entries = (size_t)B * (nbest > 0 ? nbest : 1);
        RS_HIP(ctx, hipMemsetAsync(n_ids, 0, entries * 4, (hipStream_t)stream));
        RS_HIP(ctx, hipMemsetAsync(scores, 0, entries * 4, (hipStream_t)stream));
        if (nbest > 0) {
            RS_HIP(ctx, hipMemsetAsync(norm_scores, 0, entries * 4, (hipStream_t)stream));
            RS_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)n_hyps, 1, (size_t)B, (hipStream_t)stream));
        }
        return RS_OK;
    }
    return rs_rnnt_alsd_impl(ctx, joint_enc, enc_lens, B, tp_max, beam, max_target_ratio, max_target_abs,
                             (flags & RS_ALSD_SCORE_NORM) != 0, (flags & RS_ALSD_MERGE) != 0, out_cap, ids, steps, n_ids, scores,
                             nbest, norm_scores, n_hyps, hw, hw ? graph_of : nullptr, lm, lm_alpha, workspace, workspace_bytes, (hipStream_t)stream);
}

int rs_rnnt_alsd(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                 double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids, int32_t* steps,
                 int32_t* n_ids, float* scores, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_alsd);
    return alsd_call(ctx, joint_enc, enc_lens, B, tp_max, beam, max_target_ratio, max_target_abs, flags, out_cap, ids, steps, n_ids, scores, 0, nullptr, nullptr,
                     nullptr, nullptr, nullptr, 0.0f, workspace, workspace_bytes, stream);
}

// the device hotword table of a search entry (`search` = the prefix of its messages): RS_OK and *hw the table to search with
// (nullptr: no graph in this call).  `any_table`: negative counts are refused on a table nobody points at, too (the ALSD entries).
static int hotwords_arg(rs_ctx* ctx, const char* search, bool any_table, const rs_hotwords** hw, const int32_t* graph_of) {
    const rs_hotwords* t = *hw;
    if (any_table && t && (t->n_nodes < 0 || t->n_children < 0 || t->n_graphs < 0 || t->max_level < 0))
        return rs_fail(ctx, RS_EINVAL, "%s: hotwords: negative count", search);
    if (t && graph_of && t->n_graphs > 0) {
        if (t->n_nodes < t->n_graphs || t->n_children < 0 || t->max_level < 0)
            return rs_fail(ctx, RS_EINVAL, "%s: hotwords: bad counts (%d nodes, %d children, %d graphs, max_level %d)", search, t->n_nodes,
                           t->n_children, t->n_graphs, t->max_level);
        if (!t->child_begin || !t->fail || !t->output || !t->is_end || !t->level || !t->token_score || !t->node_score ||
            !t->output_score || !t->graph_root || (t->n_children > 0 && (!t->child_tok || !t->child_node)))
            return rs_fail(ctx, RS_EINVAL, "%s: hotwords: null array", search);
    } else {
        *hw = nullptr;                                    // no graph in this call: the plain kernels, the plain bits
    }
    return RS_OK;
}

int rs_rnnt_alsd_hotwords(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                          double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids, int32_t* steps,
                          int32_t* n_ids, float* scores, const rs_hotwords* hw, const int32_t* graph_of, void* workspace,
                          size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_alsd_hotwords);
    if (int rc = hotwords_arg(ctx, "alsd", true, &hw, graph_of); rc != RS_OK) return rc;
    return alsd_call(ctx, joint_enc, enc_lens, B, tp_max, beam, max_target_ratio, max_target_abs, flags, out_cap, ids, steps, n_ids, scores, 0, nullptr, nullptr,
                     hw, graph_of, nullptr, 0.0f, workspace, workspace_bytes, stream);
}

int rs_ngram_check(const rs_ngram_host* table, char* msg, size_t msg_bytes) { return rs_ngram_check_table(table, msg, msg_bytes); }

// the device n-gram table of a search entry (`search` = the prefix of its messages): RS_OK and *lm the table to search with
// (nullptr: no model in this call)
static int ngram_arg(rs_ctx* ctx, const char* search, const rs_ngram** table, float lm_alpha) {
    const rs_ngram* lm = *table;
    if (!(lm_alpha >= 0.0f) || !isfinite(lm_alpha)) return rs_fail(ctx, RS_EINVAL, "%s: lm: lm_alpha must be a finite number >= 0", search);
    if (lm && (lm->n_nodes < 0 || lm->n_children < 0 || lm->n_logits < 0)) return rs_fail(ctx, RS_EINVAL, "%s: lm: negative count", search);
    if (lm && lm->n_nodes > 0 && lm_alpha != 0.0f) {
        if (lm->n_logits != ctx->d.n_logits)
            return rs_fail(ctx, RS_EINVAL, "%s: lm: the table is built for %d logits, the context has %d", search, lm->n_logits, ctx->d.n_logits);
        if (lm->order < 1 || lm->order > RS_NGRAM_MAX_ORDER) return rs_fail(ctx, RS_EINVAL, "%s: lm: order %d outside 1..%d", search, lm->order, (int)RS_NGRAM_MAX_ORDER);
        if (lm->start < 0 || lm->start >= lm->n_nodes) return rs_fail(ctx, RS_EINVAL, "%s: lm: start %d outside the %d nodes", search, lm->start, lm->n_nodes);
        if (!isfinite(lm->unk_logp)) return rs_fail(ctx, RS_EINVAL, "%s: lm: unk_logp is not finite", search);
        if (!lm->child_begin || !lm->root_child || !lm->logp || !lm->backoff || !lm->suffix || !lm->level ||
            (lm->n_children > 0 && (!lm->child_tok || !lm->child_node)))
            return rs_fail(ctx, RS_EINVAL, "%s: lm: null array", search);
    } else {
        *table = nullptr;                                 // no model in this call: the entry without one, the same kernels and bits
    }
    return RS_OK;
}

int rs_rnnt_alsd_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam,
                    double max_target_ratio, int max_target_abs, int flags, int out_cap, int32_t* ids, int32_t* steps,
                    int32_t* n_ids, float* scores, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm,
                    float lm_alpha, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_alsd_lm);
    if (int rc = hotwords_arg(ctx, "alsd", true, &hw, graph_of); rc != RS_OK) return rc;
    if (int rc = ngram_arg(ctx, "alsd", &lm, lm_alpha); rc != RS_OK) return rc;
    return alsd_call(ctx, joint_enc, enc_lens, B, tp_max, beam, max_target_ratio, max_target_abs, flags, out_cap, ids, steps, n_ids, scores, 0, nullptr, nullptr,
                     hw, graph_of, lm, lm_alpha, workspace, workspace_bytes, stream);
}

// ---- n-best lists of ALSD: the same dispatch with the lists as outputs ----
size_t rs_rnnt_alsd_nbest_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, double max_target_ratio, int max_target_abs, int nbest) {
    RS_GUARD_QUERY(ctx, rs_rnnt_alsd_nbest_workspace_bytes, 0);
    if (nbest < 1 || nbest > 8 || nbest > beam) return 0;
    return alsd_workspace(ctx, B, beam, tp_max, max_target_ratio, max_target_abs, true, true, nbest);      // the LM form's layout plus the list
}

int rs_rnnt_alsd_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, double max_target_ratio,
                       int max_target_abs, int flags, int nbest, int out_cap, int32_t* ids, int32_t* steps, int32_t* n_ids, float* scores,
                       float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm,
                       float lm_alpha, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_alsd_nbest);
    if (nbest < 1 || nbest > 8) return rs_fail(ctx, RS_EINVAL, "alsd: nbest must be 1..8, got %d", nbest);      // before anything is enqueued
    const int W = beam < ctx->d.n_logits - 1 ? beam : ctx->d.n_logits - 1;                                       // (the search clamps the beam)
    if (nbest > W) return rs_fail(ctx, RS_EINVAL, "alsd: nbest %d is above the beam %d", nbest, W);
    if (int rc = hotwords_arg(ctx, "alsd", true, &hw, graph_of); rc != RS_OK) return rc;
    if (int rc = ngram_arg(ctx, "alsd", &lm, lm_alpha); rc != RS_OK) return rc;
    return alsd_call(ctx, joint_enc, enc_lens, B, tp_max, beam, max_target_ratio, max_target_abs, flags, out_cap, ids, steps, n_ids, scores,
                     nbest, norm_scores, n_hyps, hw, graph_of, lm, lm_alpha, workspace, workspace_bytes, stream);
}

size_t rs_rnnt_beam_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops) {
    RS_GUARD_QUERY(ctx, rs_rnnt_beam_workspace_bytes, 0);
    if (B <= 0 || beam <= 0 || tp_max < 0 || max_pops < 0 || ctx->d.n_logits < 2) return 0;
    return rs_rnnt_beam_workspace_bytes_impl(ctx, B, beam, tp_max, max_pops, false, false);
}

// the argument checks and the dispatch of rs_rnnt_beam, rs_rnnt_beam_nbest and rs_rnnt_beam_lm (nbest >= 1: ids / frames
// [B][nbest][out_cap], n_ids / scores / norm_scores [B][nbest], n_hyps [B]; nbest = 0 and no lists: the one result; hw == nullptr and
// lm == nullptr: the plain kernels).  The callers have checked `nbest` against the beam, and the tables they take with hotwords_arg /
// ngram_arg below.
static int beam_call(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags, int max_pops,
                     int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int32_t* pops, int nbest, float* norm_scores,
                     int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm, float lm_alpha, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (B < 0 || tp_max < 0 || out_cap < 0 || max_pops < 0) return rs_fail(ctx, RS_EINVAL, "beam search: negative size");
    if (beam < 1) return rs_fail(ctx, RS_EINVAL, "beam search: beam size must be >= 1");
    if (B == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !n_ids || !scores || !pops || !workspace) return rs_fail(ctx, RS_EINVAL, "beam search: null pointer");
    if (nbest > 0 && (!norm_scores || !n_hyps)) return rs_fail(ctx, RS_EINVAL, "beam search: null pointer");
    if (tp_max == 0) {                                    // no frames anywhere: the start hypothesis, empty, score 0
        const size_t entries = (size_t)B * (nbest > 0 ? nbest : 1);
        RS_HIP(ctx, hipMemsetAsync(n_ids, 0, entries * 4, (hipStream_t)stream));
        RS_HIP(ctx, hipMemsetAsync(scores, 0, entries * 4, (hipStream_t)stream));
        RS_HIP(ctx, hipMemsetAsync(pops, 0, (size_t)B * 4, (hipStream_t)stream));
        if (nbest > 0) {
            RS_HIP(ctx, hipMemsetAsync(norm_scores, 0, entries * 4, (hipStream_t)stream));
            RS_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)n_hyps, 1, (size_t)B, (hipStream_t)stream));
        }
        return RS_OK;
    }
    return rs_rnnt_beam_impl(ctx, joint_enc, enc_lens, B, tp_max, beam, (flags & RS_BEAM_SCORE_NORM) != 0, max_pops, out_cap, ids,
                             frames, n_ids, scores, pops, nbest, norm_scores, n_hyps, hw, hw ? graph_of : nullptr, lm, lm_alpha, workspace,
                             workspace_bytes, (hipStream_t)stream);
}

int rs_rnnt_beam(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags, int max_pops,
                 int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int32_t* pops, void* workspace,
                 size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_beam);
    return beam_call(ctx, joint_enc, enc_lens, B, tp_max, beam, flags, max_pops, out_cap, ids, frames, n_ids, scores, pops, 0, nullptr,
                     nullptr, nullptr, nullptr, nullptr, 0.0f, workspace, workspace_bytes, stream);
}

// ---- n-best lists of the default beam search: the same dispatch with the lists as outputs ----
size_t rs_rnnt_beam_nbest_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest) {
    RS_GUARD_QUERY(ctx, rs_rnnt_beam_nbest_workspace_bytes, 0);
    if (B <= 0 || beam <= 0 || tp_max < 0 || max_pops < 0 || ctx->d.n_logits < 2 || nbest < 1 || nbest > 8 || nbest > beam) return 0;
    return rs_rnnt_beam_workspace_bytes_impl(ctx, B, beam, tp_max, max_pops, false, false);         // the lists live in the outputs
}

int rs_rnnt_beam_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags, int max_pops,
                       int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, float* norm_scores,
                       int32_t* n_hyps, int32_t* pops, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_beam_nbest);
    if (nbest < 1 || nbest > 8) return rs_fail(ctx, RS_EINVAL, "beam search: nbest must be 1..8, got %d", nbest);      // before anything is enqueued
    if (beam < 1) return rs_fail(ctx, RS_EINVAL, "beam search: beam size must be >= 1");
    const int bm = beam < ctx->d.n_logits ? beam : ctx->d.n_logits;                    // (the search clamps the beam to the vocabulary)
    if (nbest > bm) return rs_fail(ctx, RS_EINVAL, "beam search: nbest %d is above the beam %d", nbest, bm);
    return beam_call(ctx, joint_enc, enc_lens, B, tp_max, beam, flags, max_pops, out_cap, ids, frames, n_ids, scores, pops, nbest,
                     norm_scores, n_hyps, nullptr, nullptr, nullptr, 0.0f, workspace, workspace_bytes, stream);
}

// ---- hotwords and an n-gram LM in the default beam search: the same dispatch with the tables; nbest = 0: the one result of
// rs_rnnt_beam, nbest >= 1: the lists of rs_rnnt_beam_nbest ----
size_t rs_rnnt_beam_lm_workspace_bytes(const rs_ctx* ctx, int B, int beam, int tp_max, int max_pops, int nbest) {
    RS_GUARD_QUERY(ctx, rs_rnnt_beam_lm_workspace_bytes, 0);
    if (B <= 0 || beam <= 0 || tp_max < 0 || max_pops < 0 || ctx->d.n_logits < 2 || nbest < 0 || nbest > 8 || nbest > beam) return 0;
    return rs_rnnt_beam_workspace_bytes_impl(ctx, B, beam, tp_max, max_pops, true, true);     // the LM form's layout: room for both states
}

int rs_rnnt_beam_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, int flags, int max_pops,
                    int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, float* norm_scores, int32_t* n_hyps,
                    int32_t* pops, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm, float lm_alpha, void* workspace,
                    size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_beam_lm);
    if (nbest < 0 || nbest > 8) return rs_fail(ctx, RS_EINVAL, "beam search: nbest must be 0..8, got %d", nbest);      // before anything is enqueued
    if (beam < 1) return rs_fail(ctx, RS_EINVAL, "beam search: beam size must be >= 1");
    const int bm = beam < ctx->d.n_logits ? beam : ctx->d.n_logits;                    // (the search clamps the beam to the vocabulary)
    if (nbest > bm) return rs_fail(ctx, RS_EINVAL, "beam search: nbest %d is above the beam %d", nbest, bm);
    if (int rc = hotwords_arg(ctx, "beam search", true, &hw, graph_of); rc != RS_OK) return rc;
    if (int rc = ngram_arg(ctx, "beam search", &lm, lm_alpha); rc != RS_OK) return rc;
    return beam_call(ctx, joint_enc, enc_lens, B, tp_max, beam, flags, max_pops, out_cap, ids, frames, n_ids, scores, pops, nbest,
                     nbest > 0 ? norm_scores : nullptr, nbest > 0 ? n_hyps : nullptr, hw, graph_of, lm, lm_alpha, workspace, workspace_bytes,
                     stream);
}

size_t rs_rnnt_mbs_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_mbs_workspace_bytes, 0);
    if (B <= 0 || max_active_paths < 1 || max_active_paths > 8 || tp_max < 0 || out_cap < 0) return 0;
    return rs_rnnt_mbs_workspace_bytes_impl(ctx, B, max_active_paths, tp_max, false, false);
}

int rs_rnnt_mbs(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_mbs);
    return rs_rnnt_mbs_hotwords(ctx, joint_enc, enc_lens, B, tp_max, max_active_paths, blank_penalty, flags, out_cap, ids, frames, n_ids,
                                scores, nullptr, nullptr, workspace, workspace_bytes, stream);
}

size_t rs_rnnt_mbs_hotwords_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_mbs_hotwords_workspace_bytes, 0);
    if (B <= 0 || max_active_paths < 1 || max_active_paths > 8 || tp_max < 0 || out_cap < 0) return 0;
    return rs_rnnt_mbs_workspace_bytes_impl(ctx, B, max_active_paths, tp_max, true, false);
}

size_t rs_rnnt_mbs_lm_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_mbs_lm_workspace_bytes, 0);
    if (B <= 0 || max_active_paths < 1 || max_active_paths > 8 || tp_max < 0 || out_cap < 0) return 0;
    return rs_rnnt_mbs_workspace_bytes_impl(ctx, B, max_active_paths, tp_max, true, true);
}

// pure host code: is `t` (HOST pointers) a table the device walk may be given?  (The walk is safe on any table; a table that
// fails here would give bonuses nobody meant.)
int rs_hotwords_check(const rs_hotwords_host* t, char* msg, size_t msg_bytes) {
    auto fail = [&](const char* fmt, long long a, long long b, long long c) {
        if (msg && msg_bytes) snprintf(msg, msg_bytes, fmt, a, b, c);
        return (int)RS_EINVAL;
    };
    if (msg && msg_bytes) msg[0] = 0;
    if (!t) return fail("hotwords: null table", 0, 0, 0);
    if (t->n_nodes < 0 || t->n_children < 0 || t->n_graphs < 0 || t->max_level < 0) return fail("hotwords: negative count", 0, 0, 0);
    if (t->n_graphs == 0) return RS_OK;
    if (t->n_nodes < t->n_graphs) return fail("hotwords: %lld graphs but %lld nodes", t->n_graphs, t->n_nodes, 0);
    if (!t->child_begin || !t->fail || !t->output || !t->is_end || !t->level || !t->token_score || !t->node_score || !t->output_score ||
        !t->graph_root || (t->n_children > 0 && (!t->child_tok || !t->child_node)))
        return fail("hotwords: null array", 0, 0, 0);
    const int N = t->n_nodes, C = t->n_children;
    if (t->child_begin[0] != 0 || t->child_begin[N] != C) return fail("hotwords: child_begin must run from 0 to n_children=%lld", C, 0, 0);
    for (int g = 0; g < t->n_graphs; ++g) {
        const int r = t->graph_root[g];
        if (r < 0 || r >= N) return fail("hotwords: graph_root[%lld]=%lld outside the %lld nodes", g, r, N);
        if (t->level[r] != 0 || t->fail[r] != r) return fail("hotwords: root %lld of graph %lld must have level 0 and fail to itself", r, g, 0);
    }
    for (int n = 0; n < N; ++n) {
        const int lo = t->child_begin[n], hi = t->child_begin[n + 1];
        if (lo < 0 || hi < lo || hi > C) return fail("hotwords: child_begin[%lld..] = %lld, %lld is not an ascending range of the children", n, lo, hi);
        if (t->level[n] < 0 || t->level[n] > t->max_level) return fail("hotwords: level[%lld]=%lld outside 0..max_level=%lld", n, t->level[n], t->max_level);
        const int f = t->fail[n], o = t->output[n];
        if (f < 0 || f >= N) return fail("hotwords: fail[%lld]=%lld outside the %lld nodes", n, f, N);
        if (o < -1 || o >= N) return fail("hotwords: output[%lld]=%lld outside the %lld nodes", n, o, N);
        if (t->level[n] == 0) {
            if (f != n) return fail("hotwords: node %lld has level 0 but fails to %lld", n, f, 0);
        } else if (t->level[f] >= t->level[n]) {
            return fail("hotwords: fail[%lld]=%lld does not lower the level (%lld)", n, f, t->level[n]);
        }
        for (int c = lo; c < hi; ++c) {
            const int k = t->child_node[c];
            if (k < 0 || k >= N) return fail("hotwords: child_node[%lld]=%lld outside the %lld nodes", c, k, N);
            if (t->level[k] != t->level[n] + 1) return fail("hotwords: child %lld of node %lld is not one level below it", k, n, 0);
            if (c > lo && t->child_tok[c] <= t->child_tok[c - 1]) return fail("hotwords: the children of node %lld are not sorted ascending (entry %lld)", n, c, 0);
        }
    }
    return RS_OK;
}

// the argument checks and the dispatch of rs_rnnt_mbs, rs_rnnt_mbs_hotwords, rs_rnnt_mbs_lm (lm == nullptr: no model) and
// rs_rnnt_mbs_nbest (nbest >= 1: ids / frames [B][nbest][out_cap], n_ids / scores / norm_scores [B][nbest], n_hyps [B]; the others
// pass nbest = 0 and no lists: the one result)
static int mbs_call(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                    float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int nbest,
                    float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm, float lm_alpha,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || tp_max < 0 || out_cap < 0) return rs_fail(ctx, RS_EINVAL, "modified beam search: negative size");
    if (max_active_paths < 1 || max_active_paths > 8) return rs_fail(ctx, RS_EINVAL, "modified beam search: max_active_paths must be 1..8, got %d", max_active_paths);
    if (!(blank_penalty >= 0.0f)) return rs_fail(ctx, RS_EINVAL, "modified beam search: blank_penalty must be >= 0");
    if (B == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !frames || !n_ids || !scores || !workspace) return rs_fail(ctx, RS_EINVAL, "modified beam search: null pointer");
    if (nbest > 0 && (!norm_scores || !n_hyps)) return rs_fail(ctx, RS_EINVAL, "modified beam search: null pointer");
    if (tp_max == 0) {
        const size_t entries = (size_t)B * (nbest > 0 ? nbest : 1);
        RS_HIP(ctx, hipMemsetAsync(n_ids, 0, entries * 4, (hipStream_t)stream));
        RS_HIP(ctx, hipMemsetAsync(scores, 0, entries * 4, (hipStream_t)stream));
        if (nbest > 0) {
            RS_HIP(ctx, hipMemsetAsync(norm_scores, 0, entries * 4, (hipStream_t)stream));
            RS_HIP(ctx, hipMemsetAsync(n_hyps, 0, (size_t)B * 4, (hipStream_t)stream));
        }
        return RS_OK;
    }
    if (int rc = hotwords_arg(ctx, "modified beam search", false, &hw, graph_of); rc != RS_OK) return rc;
    return rs_rnnt_mbs_impl(ctx, joint_enc, enc_lens, B, tp_max, max_active_paths, blank_penalty, (flags & RS_MBS_LENGTH_NORM) != 0,
                            out_cap, ids, frames, n_ids, scores, nbest, norm_scores, n_hyps, hw, hw ? graph_of : nullptr, lm, lm_alpha,
                            workspace, workspace_bytes, (hipStream_t)stream);
}

int rs_rnnt_mbs_hotwords(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                         float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                         const rs_hotwords* hw, const int32_t* graph_of, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_mbs_hotwords);
    return mbs_call(ctx, joint_enc, enc_lens, B, tp_max, max_active_paths, blank_penalty, flags, out_cap, ids, frames, n_ids, scores, 0,
                    nullptr, nullptr, hw, graph_of, nullptr, 0.0f, workspace, workspace_bytes, stream);
}

int rs_rnnt_mbs_lm(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                   float blank_penalty, int flags, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                   const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm, float lm_alpha, void* workspace,
                   size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_mbs_lm);
    if (int rc = ngram_arg(ctx, "modified beam search", &lm, lm_alpha); rc != RS_OK) return rc;     // before anything is enqueued
    return mbs_call(ctx, joint_enc, enc_lens, B, tp_max, max_active_paths, blank_penalty, flags, out_cap, ids, frames, n_ids, scores, 0,
                    nullptr, nullptr, hw, graph_of, lm, lm_alpha, workspace, workspace_bytes, stream);
}

// ---- n-best lists of the modified beam search: the same dispatch with the lists as outputs ----
size_t rs_rnnt_mbs_nbest_workspace_bytes(const rs_ctx* ctx, int B, int max_active_paths, int tp_max, int out_cap, int nbest) {
    RS_GUARD_QUERY(ctx, rs_rnnt_mbs_nbest_workspace_bytes, 0);
    if (B <= 0 || max_active_paths < 1 || max_active_paths > 8 || tp_max < 0 || out_cap < 0 || nbest < 1 || nbest > max_active_paths) return 0;
    return rs_rnnt_mbs_workspace_bytes_impl(ctx, B, max_active_paths, tp_max, true, true);       // the lists live in the outputs: the LM form's layout
}

int rs_rnnt_mbs_nbest(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int max_active_paths,
                      float blank_penalty, int flags, int nbest, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores,
                      float* norm_scores, int32_t* n_hyps, const rs_hotwords* hw, const int32_t* graph_of, const rs_ngram* lm,
                      float lm_alpha, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_mbs_nbest);
    if (nbest < 1 || nbest > 8) return rs_fail(ctx, RS_EINVAL, "modified beam search: nbest must be 1..8, got %d", nbest);      // before anything is enqueued
    if (nbest > max_active_paths)
        return rs_fail(ctx, RS_EINVAL, "modified beam search: nbest %d is above max_active_paths %d", nbest, max_active_paths);
    if (int rc = ngram_arg(ctx, "modified beam search", &lm, lm_alpha); rc != RS_OK) return rc;
    return mbs_call(ctx, joint_enc, enc_lens, B, tp_max, max_active_paths, blank_penalty, flags, out_cap, ids, frames, n_ids, scores, nbest,
                    norm_scores, n_hyps, hw, graph_of, lm, lm_alpha, workspace, workspace_bytes, stream);
}

// ---- token log-probabilities of a finished search (k_rnnt_scores.hip) ----
static bool token_scores_ctx_ok(const rs_ctx* ctx) { return ctx->finalized && ctx->embed && ctx->jout_w; }

size_t rs_rnnt_token_scores_workspace_bytes(const rs_ctx* ctx, int B, int u_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_token_scores_workspace_bytes, 0);
    if (!token_scores_ctx_ok(ctx) || B <= 0 || u_cap < 0) return 0;
    return rs_rnnt_token_scores_workspace_bytes_impl(ctx, B, u_cap);
}

int rs_rnnt_token_scores(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                         const int32_t* frames, const int32_t* n_ids, int u_cap, int flags, float* logp, int32_t* top1, void* workspace,
                         size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_token_scores);
    if (!token_scores_ctx_ok(ctx)) return rs_fail(ctx, RS_EINVAL, "token scores: the context is not finalized");
    if (B < 0 || tp_max < 0 || u_cap < 0) return rs_fail(ctx, RS_EINVAL, "token scores: negative size");
    if (flags & ~RS_SCORES_FRAMES_ARE_STEPS) return rs_fail(ctx, RS_EINVAL, "token scores: unknown flag %d", flags);
    if (B == 0 || u_cap == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !frames || !n_ids || !logp || !workspace) return rs_fail(ctx, RS_EINVAL, "token scores: null pointer");
    if (workspace_bytes < rs_rnnt_token_scores_workspace_bytes_impl(ctx, B, u_cap))
        return rs_fail(ctx, RS_EINVAL, "token scores: workspace %zu < %zu", workspace_bytes, rs_rnnt_token_scores_workspace_bytes_impl(ctx, B, u_cap));
    if (tp_max == 0) return RS_OK;                         // no frames: no utterance has a token
    return rs_rnnt_token_scores_impl(ctx, joint_enc, enc_lens, B, tp_max, ids, frames, n_ids, u_cap, (flags & RS_SCORES_FRAMES_ARE_STEPS) != 0,
                                     logp, top1, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- forced alignment and transcript likelihood on the transducer lattice (k_rnnt_align.hip) ----
size_t rs_rnnt_align_workspace_bytes(const rs_ctx* ctx, int B, int tp_max, int u_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_align_workspace_bytes, 0);
    if (!token_scores_ctx_ok(ctx) || B <= 0 || tp_max < 0 || u_cap < 0 || u_cap > RS_ALIGN_U_CAP_MAX) return 0;
    return rs_rnnt_align_workspace_bytes_impl(ctx, B, tp_max, u_cap);
}

int rs_rnnt_align(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                  const int32_t* n_ids, int u_cap, int flags, float* loglik, float* best, int32_t* frames, float* logp, void* workspace,
                  size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_align);
    if (!token_scores_ctx_ok(ctx)) return rs_fail(ctx, RS_EINVAL, "align: the context is not finalized");
    if (B < 0 || tp_max < 0 || u_cap < 0) return rs_fail(ctx, RS_EINVAL, "align: negative size");
    if (flags & ~RS_ALIGN_ONE_PER_FRAME) return rs_fail(ctx, RS_EINVAL, "align: unknown flag %d", flags);
    if (u_cap > RS_ALIGN_U_CAP_MAX) return rs_fail(ctx, RS_EINVAL, "align: u_cap %d is above %d", u_cap, RS_ALIGN_U_CAP_MAX);
    if (B == 0) return RS_OK;
    if (!joint_enc || !enc_lens || !ids || !n_ids || !loglik || !best || !frames || !logp || !workspace)
        return rs_fail(ctx, RS_EINVAL, "align: null pointer");
    const size_t least = rs_rnnt_align_workspace_bytes_impl(ctx, B, tp_max, u_cap);
    if (least == 0) return rs_fail(ctx, RS_EINVAL, "align: B x tp_max x (u_cap + 1) is too large");
    if (workspace_bytes < least) return rs_fail(ctx, RS_EINVAL, "align: workspace %zu < %zu", workspace_bytes, least);
    return rs_rnnt_align_impl(ctx, joint_enc, enc_lens, B, tp_max, ids, n_ids, u_cap, (flags & RS_ALIGN_ONE_PER_FRAME) != 0, loglik, best,
                              frames, logp, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- several texts per utterance: the row-to-utterance map of both teacher-forced entries ----
size_t rs_rnnt_align_rows_workspace_bytes(const rs_ctx* ctx, int B, int R, int tp_max, int u_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_align_rows_workspace_bytes, 0);
    if (!token_scores_ctx_ok(ctx) || B <= 0 || R <= 0 || tp_max < 0 || u_cap < 0 || u_cap > RS_ALIGN_U_CAP_MAX) return 0;
    return rs_rnnt_align_rows_workspace_bytes_impl(ctx, R, tp_max, u_cap);
}

int rs_rnnt_align_rows(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt, int R,
                       const int32_t* ids, const int32_t* n_ids, int u_cap, int flags, float* loglik, float* best, int32_t* frames,
                       float* logp, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_align_rows);
    if (!token_scores_ctx_ok(ctx)) return rs_fail(ctx, RS_EINVAL, "align rows: the context is not finalized");
    if (B < 0 || R < 0 || tp_max < 0 || u_cap < 0) return rs_fail(ctx, RS_EINVAL, "align rows: negative size");
    if (flags & ~(RS_ALIGN_ONE_PER_FRAME | RS_ALIGN_NO_SHARING)) return rs_fail(ctx, RS_EINVAL, "align rows: unknown flag %d", flags);
    if (u_cap > RS_ALIGN_U_CAP_MAX) return rs_fail(ctx, RS_EINVAL, "align rows: u_cap %d is above %d", u_cap, RS_ALIGN_U_CAP_MAX);
    if (stats) stats[0] = stats[1] = 0;
    if (R == 0) return RS_OK;
    if (B == 0) return rs_fail(ctx, RS_EINVAL, "align rows: rows without an utterance");
    if (!joint_enc || !enc_lens || !row_utt || !ids || !n_ids || !loglik || !best || !frames || !logp || !workspace)
        return rs_fail(ctx, RS_EINVAL, "align rows: null pointer");
    const size_t least = rs_rnnt_align_rows_workspace_bytes_impl(ctx, R, tp_max, u_cap);
    if (least == 0) return rs_fail(ctx, RS_EINVAL, "align rows: R x tp_max x (u_cap + 1) is too large");
    if (workspace_bytes < least) return rs_fail(ctx, RS_EINVAL, "align rows: workspace %zu < %zu", workspace_bytes, least);
    return rs_rnnt_align_rows_impl(ctx, joint_enc, enc_lens, B, tp_max, row_utt, R, ids, n_ids, u_cap, (flags & RS_ALIGN_ONE_PER_FRAME) != 0,
                                   (flags & RS_ALIGN_NO_SHARING) != 0, loglik, best, frames, logp, stats, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}

size_t rs_rnnt_token_scores_rows_workspace_bytes(const rs_ctx* ctx, int B, int R, int u_cap) {
    RS_GUARD_QUERY(ctx, rs_rnnt_token_scores_rows_workspace_bytes, 0);
    if (!token_scores_ctx_ok(ctx) || B <= 0 || R <= 0 || u_cap < 0) return 0;
    return rs_rnnt_token_scores_workspace_bytes_impl(ctx, R, u_cap);
}

int rs_rnnt_token_scores_rows(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt,
                              int R, const int32_t* ids, const int32_t* frames, const int32_t* n_ids, int u_cap, int flags, float* logp,
                              int32_t* top1, void* workspace, size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_rnnt_token_scores_rows);
    if (!token_scores_ctx_ok(ctx)) return rs_fail(ctx, RS_EINVAL, "token scores rows: the context is not finalized");
    if (B < 0 || R < 0 || tp_max < 0 || u_cap < 0) return rs_fail(ctx, RS_EINVAL, "token scores rows: negative size");
    if (flags & ~RS_SCORES_FRAMES_ARE_STEPS) return rs_fail(ctx, RS_EINVAL, "token scores rows: unknown flag %d", flags);
    if (R == 0 || u_cap == 0) return RS_OK;
    if (B == 0) return rs_fail(ctx, RS_EINVAL, "token scores rows: rows without an utterance");
    if (!joint_enc || !enc_lens || !row_utt || !ids || !frames || !n_ids || !logp || !workspace)
        return rs_fail(ctx, RS_EINVAL, "token scores rows: null pointer");
    const size_t least = rs_rnnt_token_scores_workspace_bytes_impl(ctx, R, u_cap);
    if (workspace_bytes < least) return rs_fail(ctx, RS_EINVAL, "token scores rows: workspace %zu < %zu", workspace_bytes, least);
    if (tp_max == 0) return RS_OK;                         // no frames: no row has a token
    return rs_rnnt_token_scores_rows_impl(ctx, joint_enc, enc_lens, B, tp_max, row_utt, R, ids, frames, n_ids, u_cap,
                                          (flags & RS_SCORES_FRAMES_ARE_STEPS) != 0, logp, top1, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

size_t rs_ctc_align_workspace_bytes(const rs_ctx* ctx, int B, int tp_max, int c_max, int S) {
    RS_GUARD_QUERY(ctx, rs_ctc_align_workspace_bytes, 0);
    if (B <= 0 || tp_max < 0 || c_max < 2 || S < 1 || S > 8) return 0;
    return rs_ctc_align_workspace_bytes_impl(B, tp_max > 0 ? tp_max : 1, c_max);
}

int rs_ctc_align(rs_ctx* ctx, const float* probs, int ld, const int32_t* enc_lens, int B, int tp_max, const int32_t* gt,
                 const int32_t* gt_lens, int c_max, int S, int blank, int32_t* frames, int32_t* status, void* workspace,
                 size_t workspace_bytes, void* stream) {
    RS_GUARD(ctx, rs_ctc_align);
    if (B < 0 || tp_max < 0) return rs_fail(ctx, RS_EINVAL, "ctc_align: negative size");
    if (S < 1 || S > 8) return rs_fail(ctx, RS_EINVAL, "ctc_align: the longest token must have 1..8 characters, got S=%d", S);
    if (c_max < 2) return rs_fail(ctx, RS_EINVAL, "ctc_align: c_max must be >= 2 (a ground truth has at least its two separators), got %d", c_max);
    if (ld < 1 || blank < 0 || blank >= ld) return rs_fail(ctx, RS_EINVAL, "ctc_align: blank %d outside the row pitch %d", blank, ld);
    if (B == 0) return RS_OK;
    if (!probs || !enc_lens || !gt || !gt_lens || !frames || !status || !workspace) return rs_fail(ctx, RS_EINVAL, "ctc_align: null pointer");
    const size_t need = rs_ctc_align_workspace_bytes(ctx, B, tp_max, c_max, S);
    if (workspace_bytes < need)
        return rs_fail(ctx, RS_EINVAL, "ctc_align: workspace of %zu bytes, rs_ctc_align_workspace_bytes asks for %zu", workspace_bytes, need);
    return rs_ctc_align_impl(ctx, probs, ld, enc_lens, B, tp_max, gt, gt_lens, c_max, S, blank, frames, status, workspace, (hipStream_t)stream);
}

int rs_ctc_find_blank(rs_ctx* ctx, const float* blank_prob, const int32_t* enc_lens, const int32_t* n_samples, int B, int tp_max,
                      float threshold, int32_t* cuts, void* stream) {
    RS_GUARD(ctx, rs_ctc_find_blank);
    if (B <= 0 || tp_max <= 0) return rs_fail(ctx, RS_EINVAL, "ctc_find_blank: B and tp_max must be positive, got B=%d tp_max=%d", B, tp_max);
    if (!blank_prob || !enc_lens || !n_samples || !cuts) return rs_fail(ctx, RS_EINVAL, "ctc_find_blank: null pointer");
    return rs_ctc_find_blank_impl(ctx, blank_prob, enc_lens, n_samples, B, tp_max, threshold, cuts, (hipStream_t)stream);
}

int rs_resample(rs_ctx* ctx, const float* x, const int64_t* row_off, const int32_t* row_len, int B, int channels, const float* table, int up,
                int down, int numtaps, float* out, int64_t out_pitch, int out_offset, int32_t* out_lens, void* stream) {
    RS_GUARD(ctx, rs_resample);
    if (B < 0 || channels < 1) return rs_fail(ctx, RS_EINVAL, "resample: B must be >= 0 and channels >= 1, got B=%d channels=%d", B, channels);
    if (up < 1 || down < 1 || up > (1 << 24) || down > (1 << 24))
        return rs_fail(ctx, RS_EINVAL, "resample: up and down must lie in 1..2^24, got %d/%d", up, down);
    if (numtaps < 1 || numtaps > (1 << 24) || numtaps % 2 == 0)
        return rs_fail(ctx, RS_EINVAL, "resample: numtaps must be odd and at most 2^24, got %d", numtaps);
    if (out_offset < 0 || out_pitch < out_offset)
        return rs_fail(ctx, RS_EINVAL, "resample: out_offset %d outside the row pitch %lld", out_offset, (long long)out_pitch);
    if (B == 0) return RS_OK;
    if (!x || !row_off || !row_len || !table || !out || !out_lens) return rs_fail(ctx, RS_EINVAL, "resample: null pointer");
    return rs_resample_impl(ctx, x, row_off, row_len, B, channels, table, up, down, numtaps, out, (long long)out_pitch, out_offset, out_lens,
                            (hipStream_t)stream);
}

// the avsr feature kernels run without a context: select `device` for the launch, and leave the caller's current device as it was
namespace {
struct rs_device_scope {
    int cur = -1, dev;
    bool ok;
    explicit rs_device_scope(int device) : dev(device) {
        ok = hipGetDevice(&cur) == hipSuccess && (cur == dev || hipSetDevice(dev) == hipSuccess);
    }
    ~rs_device_scope() {
        if (ok && cur != dev) (void)hipSetDevice(cur);
    }
};
}  // namespace

int rs_avsr_logfbank(int device, const float* audio, const int64_t* row_off, const int32_t* row_len, int B, int T, int stack, int normalize,
                     const float* twiddle, const int32_t* fb_idx, const float* fb_w, float* out, void* stream) {
    if (B < 0 || T < 1 || stack < 1 || stack > 8) return RS_EINVAL;
    if (B == 0) return RS_OK;
    if (!audio || !row_off || !row_len || !twiddle || !fb_idx || !fb_w || !out) return RS_EINVAL;
    if ((uintptr_t)twiddle & 7) return RS_EINVAL;
    rs_device_scope scope(device);
    if (!scope.ok) return RS_EHIP;
    return rs_avsr_logfbank_launch(audio, row_off, row_len, B, T, stack, normalize != 0, twiddle, fb_idx, fb_w, out, (hipStream_t)stream) == hipSuccess
               ? RS_OK : RS_EHIP;
}

int rs_avsr_pixels(int device, const uint8_t* frames, int64_t n_frames, int H, int W, int channels, const int32_t* frame_idx, int idx_pitch,
                   int B, int T, int crop, int top, int left, const float* lut, float* out, void* stream) {
    if (B < 0 || T < 1 || n_frames < 0 || H < 1 || W < 1 || crop < 4 || crop % 4) return RS_EINVAL;   // 16-byte stores: four pixels of a row
    if (channels != 1 && channels != 3) return RS_EINVAL;
    if (top < 0 || left < 0 || crop > H || crop > W || top > H - crop || left > W - crop) return RS_EINVAL;
    if (idx_pitch < T) return RS_EINVAL;
    if (B == 0) return RS_OK;
    if (!frames || !frame_idx || !lut || !out) return RS_EINVAL;
    if (((uintptr_t)frames & 3) || ((uintptr_t)out & 15)) return RS_EINVAL;
    rs_device_scope scope(device);
    if (!scope.ok) return RS_EHIP;
    return rs_avsr_pixels_launch(frames, (long long)n_frames, H, W, channels, frame_idx, idx_pitch, B, T, crop, top, left, lut, out,
                                 (hipStream_t)stream) == hipSuccess
               ? RS_OK : RS_EHIP;
}

// ---- profiling -------------------------------------------------------------------------------------
int rs_profile_enable(rs_ctx* ctx, int class_mask) {
    RS_GUARD(ctx, rs_profile_enable);
    ctx->prof_mask = class_mask;
    return RS_OK;
}
int rs_profile_reset(rs_ctx* ctx) {
    RS_GUARD(ctx, rs_profile_reset);
    for (auto& p : ctx->prof) { p.used = 0; p.flops = p.bytes = p.ms_acc = 0; p.launches = 0; p.detail.clear(); p.read = 0; }
    return RS_OK;
}
int rs_profile_read(rs_ctx* ctx, int klass, double* ms, int64_t* launches, double* flops, double* bytes) {
    RS_GUARD(ctx, rs_profile_read);
    if (klass <= 0) return RS_EINVAL;
    rs_prof_slot& p = ctx->prof[rs_prof_class_index(klass)];
    double total = p.ms_acc;
    for (size_t i = 0; i + 1 < p.used; i += 2) {
        RS_HIP(ctx, hipEventSynchronize(p.ev[i + 1]));
        float t = 0;
        RS_HIP(ctx, hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]));
        total += t;
        if (p.read < p.detail.size()) p.detail[p.read++].ms = t;      // launches are bracketed and read in the same order
    }
    p.ms_acc = total;
    p.used = 0;
    if (ms) *ms = total;
    if (launches) *launches = p.launches;
    if (flops) *flops = p.flops;
    if (bytes) *bytes = p.bytes;
    return RS_OK;
}

int rs_profile_read_launches(rs_ctx* ctx, int klass, int32_t* shapes, double* flops, float* ms, int cap, int* n_out) {
    RS_GUARD(ctx, rs_profile_read_launches);
    if (klass <= 0 || cap < 0 || !n_out) return RS_EINVAL;
    if (int rc = rs_profile_read(ctx, klass, nullptr, nullptr, nullptr, nullptr); rc != RS_OK) return rc;   // folds pending events in
    const rs_prof_slot& p = ctx->prof[rs_prof_class_index(klass)];
    const int n = (int)p.read < cap ? (int)p.read : cap;
    for (int i = 0; i < n; ++i) {
        const rs_prof_launch& l = p.detail[i];
        if (shapes) { shapes[4 * i] = l.M; shapes[4 * i + 1] = l.N; shapes[4 * i + 2] = l.K; shapes[4 * i + 3] = l.flags; }
        if (flops) flops[i] = l.flops;
        if (ms) ms[i] = l.ms;
    }
    *n_out = (int)p.read;
    return RS_OK;
}

// ---- single-operator entry points --------------------------------------------------------------------
int rs_gemm_bf16(rs_ctx* ctx, const uint16_t* A, int lda, const uint16_t* W, int ldw, void* out, int ldc, int M, int N,
                 int K, int flags, const float* bias, float alpha, const float* residual, const int32_t* mask_lens,
                 int mask_rows_per_step, int mask_steps, void* stream) {
    RS_GUARD(ctx, rs_gemm_bf16);
    if (M == 0 || N == 0) return RS_OK;
    if (!A || !W || !out) return rs_fail(ctx, RS_EINVAL, "gemm: null pointer");
    rs_gemm_args g{A, lda, W, ldw, out, ldc, M, N, K, flags, bias, alpha, residual, mask_lens, mask_rows_per_step, mask_steps};
    return rs_launch_gemm(ctx, g, (hipStream_t)stream);
}

int rs_gemm_f32(rs_ctx* ctx, const float* A, int lda, const float* W, int ldw, float* out, int ldc, int M, int N, int K, int flags,
                const float* bias, float alpha, const float* residual, const int32_t* mask_lens, int mask_rows_per_step,
                int mask_steps, void* stream) {
    RS_GUARD(ctx, rs_gemm_f32);
    if (M == 0 || N == 0) return RS_OK;
    if (!A || !W || !out) return rs_fail(ctx, RS_EINVAL, "gemm_f32: null pointer");
    return rs_launch_gemm_f32(ctx, A, lda, W, ldw, out, ldc, M, N, K, flags, bias, alpha, residual, mask_lens, mask_rows_per_step,
                              mask_steps, (hipStream_t)stream);
}

int rs_relpos_attention_f32(rs_ctx* ctx, const float* qkv, const float* pos, const float* bias_u, const float* bias_v,
                            const int32_t* lens, int B, int T, float* ctx_out, void* stream) {
    RS_GUARD(ctx, rs_relpos_attention_f32);
    if (!qkv || !pos || !bias_u || !bias_v || !lens || !ctx_out) return rs_fail(ctx, RS_EINVAL, "attention_f32: null pointer");
    return rs_launch_attention_f32(ctx, qkv, pos, bias_u, bias_v, lens, B, T, ctx_out, (hipStream_t)stream);
}

int rs_glu_dwconv_silu_f32(rs_ctx* ctx, const float* x, const float* dw_w, const float* dw_b, const int32_t* lens, int B, int T,
                           int d, int k, float* out, void* stream) {
    RS_GUARD(ctx, rs_glu_dwconv_silu_f32);
    if (!x || !dw_w || !dw_b || !lens || !out) return rs_fail(ctx, RS_EINVAL, "glu_dwconv_f32: null pointer");
    return rs_launch_glu_dwconv_f32(ctx, x, dw_w, dw_b, lens, B, T, d, k, out, (hipStream_t)stream);
}

int rs_layernorm(rs_ctx* ctx, const float* x, const float* gamma, const float* beta, int M, int d, float eps,
                 uint16_t* out_bf16, float* out_f32, void* stream) {
    RS_GUARD(ctx, rs_layernorm);
    if (!x || !gamma || !beta) return rs_fail(ctx, RS_EINVAL, "layernorm: null pointer");
    return rs_launch_layernorm(ctx, x, gamma, beta, M, d, eps, out_bf16, out_f32, (hipStream_t)stream);
}

int rs_relpos_attention(rs_ctx* ctx, const uint16_t* qkv, const uint16_t* pos, const float* bias_u, const float* bias_v,
                        const int32_t* lens, int B, int T, uint16_t* ctx_out, void* stream) {
    RS_GUARD(ctx, rs_relpos_attention);
    if (!qkv || !pos || !bias_u || !bias_v || !lens || !ctx_out) return rs_fail(ctx, RS_EINVAL, "attention: null pointer");
    return rs_launch_attention(ctx, qkv, pos, bias_u, bias_v, lens, B, T, ctx_out, (hipStream_t)stream);
}

int rs_glu_dwconv_silu(rs_ctx* ctx, const uint16_t* x, const float* dw_w, const float* dw_b, const int32_t* lens, int B,
                       int T, int d, int k, uint16_t* out, void* stream) {
    RS_GUARD(ctx, rs_glu_dwconv_silu);
    if (!x || !dw_w || !dw_b || !lens || !out) return rs_fail(ctx, RS_EINVAL, "glu_dwconv: null pointer");
    return rs_launch_glu_dwconv(ctx, x, RS_GLU_HALVES, dw_w, dw_b, lens, B, T, d, k, out, (hipStream_t)stream);
}

int rs_glu_dwconv_silu_layout(rs_ctx* ctx, const uint16_t* x, int layout, const float* dw_w, const float* dw_b,
                              const int32_t* lens, int B, int T, int d, int k, uint16_t* out, void* stream) {
    RS_GUARD(ctx, rs_glu_dwconv_silu_layout);
    if (!x || !dw_w || !dw_b || !lens || !out) return rs_fail(ctx, RS_EINVAL, "glu_dwconv: null pointer");
    return rs_launch_glu_dwconv(ctx, x, layout, dw_w, dw_b, lens, B, T, d, k, out, (hipStream_t)stream);
}


}  // extern "C"
