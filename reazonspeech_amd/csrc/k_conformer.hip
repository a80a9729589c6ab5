// k_conformer.hip — the Conformer family (rs_create: NeMo's FastConformer and ESPnet's Conformer, told apart by rs_dims switches):
// its state (rs_common.h: rs_conformer), finalize, workspace plan and the two encoder call sequences — the bf16 throughput mode and,
// side by side with it, the float32 parity mode (kernels: k_f32.hip).  Host code only; the kernels live in the other k_*.hip files.
#include <algorithm>

#include "rs_common.h"

extern "C" int rs_create(rs_ctx** out, int device, const rs_dims* dims) {
    if (!out || !dims) return RS_EINVAL;
    *out = nullptr;
    rs_ctx* ctx = new (std::nothrow) rs_ctx();
    rs_conformer* state = ctx ? new (std::nothrow) rs_conformer() : nullptr;
    if (!state) { delete ctx; return RS_EINVAL; }
    rs_conformer& cf = *state;
    ctx->family = RS_FAM_CONFORMER;
    ctx->state.reset(state);
    ctx->device = device;
    ctx->d = *dims;
    const rs_dims& d = ctx->d;
    int rc = RS_OK;
    if (d.n_heads <= 0 || d.d_model % d.n_heads || (d.d_model / d.n_heads != 128 && d.d_model / d.n_heads != 64))
        rc = rs_fail(ctx, RS_EINVAL, "head_dim must be 128 or 64 (d_model %d, heads %d)", d.d_model, d.n_heads);
    else if (d.d_model % 256 || d.ff_dim % 64) rc = rs_fail(ctx, RS_EINVAL, "d_model %% 256, ff_dim %% 64 required");
    else if (d.sub_stages < 2 || d.sub_stages > 4) rc = rs_fail(ctx, RS_EINVAL, "2..4 subsampling stages supported");
    else if (d.n_layers < 1) rc = rs_fail(ctx, RS_EINVAL, "n_layers");
    else if (d.pred_layers < 1 || d.pred_layers > 4) rc = rs_fail(ctx, RS_EINVAL, "pred_layers");
    else if ((unsigned)d.frontend_kind > 1u /* 2 = kaldi fbank: rs_k2_create only */ || (unsigned)d.sub_kind > 1u || (unsigned)d.final_norm > 1u || (unsigned)d.joint_act > 1u)
        rc = rs_fail(ctx, RS_EINVAL, "model family switches must be 0 or 1");
    else if (d.sub_kind == 1 && (d.sub_stages != 2 || d.sub_channels % 64)) rc = rs_fail(ctx, RS_EINVAL, "Conv2dSubsampling: x4 (two stages), channels %% 64");
    else if (d.frontend_kind == 1 && d.preemph != 0.0f) rc = rs_fail(ctx, RS_EINVAL, "the ESPnet front-end has no pre-emphasis");
    else if (d.ctc_vocab < 0) rc = rs_fail(ctx, RS_EINVAL, "ctc_vocab < 0");
    if (rc != RS_OK) { *out = ctx; return rc; }  // caller can read rs_last_error, then rs_destroy
    cf.head_dim = d.d_model / d.n_heads;
    int f = d.n_mels;
    for (int s = 0; s < d.sub_stages; ++s) f = rs_conv_len(f, d.sub_kind);
    cf.sub_freq = f;
    if (hipSetDevice(device) != hipSuccess) { *out = ctx; return rs_fail(ctx, RS_EHIP, "hipSetDevice(%d) failed", device); }
    *out = ctx;
    return RS_OK;
}

int rs_conformer_finalize_impl(rs_ctx* ctx) {
    rs_conformer& cf = *rs_conformer_of(ctx);
    const rs_dims& d = ctx->d;
    rs_weights r(ctx);
    const size_t C = d.sub_channels, dm = d.d_model, ff = d.ff_dim, H = d.pred_hidden, J = d.joint_hidden, V = d.n_logits;
    r.get("fe.window", (size_t)d.win_length, ctx->fe_window);
    r.get("fe.twiddle", (size_t)512, ctx->fe_twiddle);
    r.get("fe.fb_idx", (size_t)d.n_mels * 2, ctx->fe_fb_idx);
    r.get("fe.fb_w", (size_t)d.n_mels * 32, ctx->fe_fb_w);
    r.get("sub.conv0.w", 9 * C, cf.sub_conv0_w);
    r.get("sub.conv0.b", C, cf.sub_conv0_b);
    if (d.frontend_kind == 1) { r.get("fe.mvn_mean", (size_t)d.n_mels, cf.fe_mvn_mean); r.get("fe.mvn_istd", (size_t)d.n_mels, cf.fe_mvn_istd); }
    if (d.sub_kind == 1) { r.get("sub.conv1.w", C * 9 * C, cf.sub_conv1_w); r.get("sub.conv1.b", C, cf.sub_conv1_b); }
    if (d.final_norm) { r.get("final_norm.g", dm, cf.final_norm_g); r.get("final_norm.b", dm, cf.final_norm_b); }
    if (d.ctc_vocab > 0) { r.get("ctc.w", (size_t)rs_ctc_pad(d.ctc_vocab) * dm, cf.ctc_w); r.get("ctc.b", (size_t)rs_ctc_pad(d.ctc_vocab), cf.ctc_b); }
    for (int s = 1; s < d.sub_stages && d.sub_kind == 0; ++s) {
        const std::string p = "sub.dw" + std::to_string(s), q = "sub.pw" + std::to_string(s);
        r.get(p + ".w", 9 * C, cf.sub_dw_w[s - 1]);
        r.get(p + ".b", C, cf.sub_dw_b[s - 1]);
        r.get(q + ".w", C * C, cf.sub_pw_w[s - 1]);
        r.get(q + ".b", C, cf.sub_pw_b[s - 1]);
    }
    r.get("sub.out.w", dm * C * cf.sub_freq, cf.sub_out_w);
    r.get("sub.out.b", dm, cf.sub_out_b);
    cf.layers.assign(d.n_layers, rs_layer_w{});
    for (int i = 0; i < d.n_layers; ++i) {
        rs_layer_w& L = cf.layers[i];
        const std::string p = "L" + std::to_string(i) + ".";
        r.get(p + "ln_ff1.g", dm, L.ln_ff1_g); r.get(p + "ln_ff1.b", dm, L.ln_ff1_b);
        r.get(p + "ff1.w1", ff * dm, L.ff1_w1); r.get(p + "ff1.b1", ff, L.ff1_b1);
        r.get(p + "ff1.w2", dm * ff, L.ff1_w2); r.get(p + "ff1.b2", dm, L.ff1_b2);
        r.get(p + "ln_att.g", dm, L.ln_att_g); r.get(p + "ln_att.b", dm, L.ln_att_b);
        r.get(p + "att.qkv.w", 3 * dm * dm, L.qkv_w); r.get(p + "att.qkv.b", 3 * dm, L.qkv_b);
        r.get(p + "att.out.w", dm * dm, L.out_w); r.get(p + "att.out.b", dm, L.out_b);
        r.get(p + "att.pos.w", dm * dm, L.pos_w);
        r.get(p + "att.bias_u", dm, L.bias_u); r.get(p + "att.bias_v", dm, L.bias_v);
        r.get(p + "ln_conv.g", dm, L.ln_conv_g); r.get(p + "ln_conv.b", dm, L.ln_conv_b);
        r.get(p + "conv.pw1.w", 2 * dm * dm, L.pw1_w); r.get(p + "conv.pw1.b", 2 * dm, L.pw1_b);
        r.get(p + "conv.dw.w", (size_t)d.conv_kernel * dm, L.dw_w); r.get(p + "conv.dw.b", dm, L.dw_b);
        r.get(p + "conv.pw2.w", dm * dm, L.pw2_w); r.get(p + "conv.pw2.b", dm, L.pw2_b);
        r.get(p + "ln_ff2.g", dm, L.ln_ff2_g); r.get(p + "ln_ff2.b", dm, L.ln_ff2_b);
        r.get(p + "ff2.w1", ff * dm, L.ff2_w1); r.get(p + "ff2.b1", ff, L.ff2_b1);
        r.get(p + "ff2.w2", dm * ff, L.ff2_w2); r.get(p + "ff2.b2", dm, L.ff2_b2);
        r.get(p + "ln_out.g", dm, L.ln_out_g); r.get(p + "ln_out.b", dm, L.ln_out_b);
    }
    r.get("joint.enc.w", J * dm, ctx->jenc_w); r.get("joint.enc.b", J, ctx->jenc_b);
    r.get("pred.embed", V * H, ctx->embed);
    for (int l = 0; l < d.pred_layers; ++l) {
        const std::string p = "pred.lstm" + std::to_string(l);
        r.get(p + ".w", 4 * H * 2 * H, ctx->lstm_w[l]);
        r.get(p + ".b", 4 * H, ctx->lstm_b[l]);
    }
    r.get("joint.pred.w", J * H, ctx->jpred_w); r.get("joint.pred.b", J, ctx->jpred_b);
    r.get("joint.out.w", ((V + 15) / 16 * 16) * J, ctx->jout_w); r.get("joint.out.b", V, ctx->jout_b);   // fragment-major, rows padded to 16
    if (!r.ok()) return r.fail(ctx);
    // optional: the screened joint's operands (bf16 [Vpad][J] row-major, f32 [V][J] row-major, bias padded with -3e38,
    // the largest row norm).  All four or none; without them the decode loop evaluates every column in exact f32.
    {
        rs_get_screened_joint(ctx, r);
        if (!r.ok()) return r.fail(ctx);
        for (int l = 0; l < d.pred_layers; ++l) {
            const std::string nm = "pred.lstm" + std::to_string(l) + ".w4";
            ctx->lstm_w4[l] = nullptr;
            if (r.has(nm)) { r.get(nm, 4 * H * 2 * H, ctx->lstm_w4[l]); if (!r.ok()) return r.fail(ctx); }
        }
        // the environment's values of these rows are defaults: applied ONCE per context (rs_finalize runs again after every
        // rs_set_tensor, e.g. when the position tables grow; a value chosen with rs_set_option must survive that)
        if (!ctx->env_read) {
            ctx->env_read = true;
            if (rs_knob_given(RS_KNOB_DECODE_SCREEN)) ctx->decode_screen = rs_knob(RS_KNOB_DECODE_SCREEN) != 0;
            if (rs_knob_given(RS_KNOB_DECODE_NARROW)) ctx->decode_narrow = rs_knob(RS_KNOB_DECODE_NARROW) != 0;
            if (rs_knob_given(RS_KNOB_FUSE_GLU)) cf.fuse_glu = rs_knob(RS_KNOB_FUSE_GLU) != 0;
            if (rs_knob_given(RS_KNOB_DEFER_OUT_NORM)) cf.defer_out_norm = rs_knob(RS_KNOB_DEFER_OUT_NORM) != 0;
        }
    }
    // optional: the float32 parity mode's dense weights ("<name>.f32", unrounded, the layouts of the bf16 tensors except
    // conv.pw1, which keeps NeMo's own row order) and its position table.  All or none.
    ctx->has_f32 = false;
    if (r.has("sub.out.w.f32")) {
        rs_f32_weights& w = cf.f32;
        for (int s = 1; s < d.sub_stages && d.sub_kind == 0; ++s) r.get("sub.pw" + std::to_string(s) + ".w.f32", C * C, w.sub_pw_w[s - 1]);
        if (d.sub_kind == 1) r.get("sub.conv1.w.f32", C * 9 * C, w.sub_conv1_w);
        if (d.ctc_vocab > 0) r.get("ctc.w.f32", (size_t)rs_ctc_pad(d.ctc_vocab) * dm, w.ctc_w);
        r.get("sub.out.w.f32", dm * C * cf.sub_freq, w.sub_out_w);
        w.layers.assign(d.n_layers, rs_layer_w32{});
        for (int i = 0; i < d.n_layers; ++i) {
            rs_layer_w32& L = w.layers[i];
            const std::string p = "L" + std::to_string(i) + ".";
            r.get(p + "ff1.w1.f32", ff * dm, L.ff1_w1); r.get(p + "ff1.w2.f32", dm * ff, L.ff1_w2);
            r.get(p + "ff2.w1.f32", ff * dm, L.ff2_w1); r.get(p + "ff2.w2.f32", dm * ff, L.ff2_w2);
            r.get(p + "att.qkv.w.f32", 3 * dm * dm, L.qkv_w); r.get(p + "att.out.w.f32", dm * dm, L.out_w);
            r.get(p + "att.pos.w.f32", dm * dm, L.pos_w);
            r.get(p + "conv.pw1.w.f32", 2 * dm * dm, L.pw1_w); r.get(p + "conv.pw1.b.f32", 2 * dm, L.pw1_b);
            r.get(p + "conv.pw2.w.f32", dm * dm, L.pw2_w);
        }
        r.get("joint.enc.w.f32", J * dm, w.jenc_w);
        if (!r.ok()) return r.fail(ctx);
        auto pt = ctx->tensors.find("pos.table.f32");
        if (pt == ctx->tensors.end()) return rs_fail(ctx, RS_EMISSING, "weight tensor 'pos.table.f32' was not registered");
        const size_t rowf = dm * sizeof(float);
        if (pt->second.second % rowf || !((pt->second.second / rowf) & 1) || ((uintptr_t)pt->second.first & 15))
            return rs_fail(ctx, RS_EINVAL, "pos.table.f32 must be 16-byte aligned f32 [2*Tcap-1][d_model]");
        w.pos_table = reinterpret_cast<const float*>(pt->second.first);
        w.pos_table_bytes = pt->second.second;
        ctx->has_f32 = true;
    }
    if (ctx->precision_f32 && !ctx->has_f32) ctx->precision_f32 = 0;     // (the tensors were re-registered without the f32 set)
    auto it = ctx->tensors.find("pos.table");
    if (it == ctx->tensors.end()) return rs_fail(ctx, RS_EMISSING, "weight tensor 'pos.table' was not registered");
    const size_t rowb = dm * sizeof(uint16_t);
    if (it->second.second % rowb || !((it->second.second / rowb) & 1))
        return rs_fail(ctx, RS_EINVAL, "pos.table must be bf16 [2*Tcap-1][d_model]");
    cf.pos_table = reinterpret_cast<const uint16_t*>(it->second.first);
    cf.pos_table_bytes = it->second.second;
    // optional derived weights: the position table already projected by each layer's linear_pos
    // (it depends on nothing but the weights, so a caller can compute it once with rs_gemm_bf16)
    for (int i = 0; i < d.n_layers; ++i) {
        auto pp = ctx->tensors.find("L" + std::to_string(i) + ".att.pos_proj");
        if (pp == ctx->tensors.end()) { cf.layers[i].pos_proj = nullptr; continue; }
        if (pp->second.second != it->second.second || ((uintptr_t)pp->second.first & 15))
            return rs_fail(ctx, RS_EINVAL, "L%d.att.pos_proj must be 16-byte aligned and as large as pos.table", i);
        cf.layers[i].pos_proj = reinterpret_cast<const uint16_t*>(pp->second.first);
    }
    ctx->finalized = true;
    return RS_OK;
}

namespace {

struct EncPlan {
    int T[5], F[5];  // per stage time / freq extents (index 0 = mel)
    int32_t* lens;
    uint16_t *sa, *col, *sb;   // col: the gathered patch matrix ($RS_SUB_IM2COL), else nullptr
    float* x;
    uint16_t *hn, *big, *ctxb, *posp;
    float *stats, *ctc;        // ctc: nullptr without a CTC head
    int chunk;       // Conv2dSubsampling: utterances per pass of conv0 / patch gather / dense-conv GEMM
};
constexpr size_t ENC_SLACK = 256;

EncPlan plan_encoder(const rs_ctx* ctx, int B, int t_max, rs_arena& a) {
    const rs_dims& d = ctx->d;
    EncPlan p{};
    p.T[0] = t_max; p.F[0] = d.n_mels;
    for (int s = 1; s <= d.sub_stages; ++s) { p.T[s] = rs_conv_len(p.T[s - 1], d.sub_kind); p.F[s] = rs_conv_len(p.F[s - 1], d.sub_kind); }
    const size_t C = d.sub_channels, dm = d.d_model;
    const size_t Tp = p.T[d.sub_stages] > 0 ? p.T[d.sub_stages] : 1, M = (size_t)B * Tp;
    size_t widest = (size_t)d.ff_dim;
    if (3 * dm > widest) widest = 3 * dm;
    p.lens = a.take<int32_t>((size_t)4 * B);
    p.chunk = B;
    if (d.sub_kind == 1) {
        // sa = conv0 output of ONE chunk of utterances [chunk][T1][F1][C]; sb = the dense conv's output of the WHOLE batch
        // [B][T2][F2][C].  The GEMM reads the 3 x 3 patches in place (rs_gemm_args.conv_C): the chunk keeps sa within the
        // kernel's 32-bit offsets (2 GiB here).  With $RS_SUB_IM2COL (tests/test_gpu_knobs.py runs it: the gathered patch matrix
        // col [chunk * T2 * F2][9C], the first form — 16 GB written and read again per 256 x 10 s, 4.2 ms) the chunk keeps col
        // near 1 GiB instead.
        const bool gathered = rs_knob(RS_KNOB_SUB_IM2COL) != 0;
        const size_t T1 = p.T[1] > 0 ? p.T[1] : 1, T2 = p.T[2] > 0 ? p.T[2] : 1;
        const rs_sub_chunk sa = rs_sub_chunk_rule(T1 * p.F[1] * C * 2, (size_t)1 << 31, T1, B);   // (grid limit of the conv0 / gather kernels)
        const rs_sub_chunk col = rs_sub_chunk_rule(T2 * p.F[2] * 9 * C * 2, (size_t)1 << 30, T1, B);
        p.chunk = gathered ? col.chunk : sa.chunk;
        p.sa = a.take<uint16_t>(sa.reserve / 2);
        p.col = gathered ? a.take<uint16_t>(col.reserve / 2) : nullptr;
        p.sb = a.take<uint16_t>((size_t)B * T2 * p.F[2] * C);
    } else {
        const size_t sub_elems = (size_t)B * p.T[2] * p.F[2] * C;  // stage-2 extent is the largest stored one
        p.sa = a.take<uint16_t>(sub_elems);
        p.sb = a.take<uint16_t>(sub_elems);
    }
    p.x = a.take<float>(M * dm);
    p.hn = a.take<uint16_t>(M * dm);
    p.big = a.take<uint16_t>(M * widest);
    p.ctxb = a.take<uint16_t>(M * dm);
    p.posp = a.take<uint16_t>((2 * Tp) * dm);
    p.stats = a.take<float>(M * 2);                     // (mean, rstd) per row of a deferred output norm
    p.ctc = d.ctc_vocab > 0 ? a.take<float>(M * (size_t)rs_ctc_pad(d.ctc_vocab)) : nullptr;   // CTC logits when only the blank column is wanted
    return p;
}

struct EncPlanF32 {
    int T[5], F[5];
    int32_t* lens;
    float *sa, *col, *sb, *x, *hn, *big, *ctxb, *posp, *ctc;   // ctc: nullptr without a CTC head
    int chunk;       // Conv2dSubsampling: utterances per pass of conv0 / patch gather / dense-conv GEMM
};
constexpr size_t ENC_F32_SLACK = 256;

EncPlanF32 plan_f32(const rs_ctx* ctx, int B, int t_max, rs_arena& a) {
    const rs_dims& d = ctx->d;
    EncPlanF32 p{};
    p.T[0] = t_max; p.F[0] = d.n_mels;
    for (int s = 1; s <= d.sub_stages; ++s) { p.T[s] = rs_conv_len(p.T[s - 1], d.sub_kind); p.F[s] = rs_conv_len(p.F[s - 1], d.sub_kind); }
    const size_t C = d.sub_channels, dm = d.d_model;
    const size_t Tp = p.T[d.sub_stages] > 0 ? p.T[d.sub_stages] : 1, M = (size_t)B * Tp;
    size_t widest = (size_t)d.ff_dim;
    if (3 * dm > widest) widest = 3 * dm;
    p.lens = a.take<int32_t>((size_t)4 * B);
    p.chunk = B;
    if (d.sub_kind == 1) {
        // the pieces of plan_encoder with float32 elements: conv0 output and 3x3 patches of ONE chunk of utterances, the
        // dense conv's output of the whole batch.  Each chunked buffer stays within 1 GiB and is reserved by rs_sub_chunk_rule's
        // bound, and the chunk is the smaller of the two rules' so that both reserves cover it.  CONDITION for the chunk to be the
        // patch matrix's alone, as it was before the conv0 buffer had a rule of its own: T1 F1 <= 9 T2 F2.  It holds for 80 mels
        // (F1 39, F2 19, T1 <= 4 T2: 39 T1 <= 156 T2 < 171 T2); a front end of very few features (F1 3, F2 1 at T1 4) would run
        // more, smaller passes than the patch rule asks for, with the same results.
        const size_t T1 = p.T[1] > 0 ? p.T[1] : 1, T2 = p.T[2] > 0 ? p.T[2] : 1;
        const rs_sub_chunk col = rs_sub_chunk_rule(T2 * p.F[2] * 9 * C * 4, (size_t)1 << 30, T2, B);
        const rs_sub_chunk sa = rs_sub_chunk_rule(T1 * p.F[1] * C * 4, (size_t)1 << 30, T2, B);
        p.chunk = std::min(col.chunk, sa.chunk);
        p.sa = a.take<float>(sa.reserve / 4);
        p.col = a.take<float>(col.reserve / 4);
        p.sb = a.take<float>((size_t)B * T2 * p.F[2] * C);
    } else {
        const size_t sub_elems = (size_t)B * p.T[2] * p.F[2] * C;
        p.sa = a.take<float>(sub_elems);
        p.sb = a.take<float>(sub_elems);
    }
    p.x = a.take<float>(M * dm);
    p.hn = a.take<float>(M * dm);
    p.big = a.take<float>(M * widest);
    p.ctxb = a.take<float>(M * dm);
    p.posp = a.take<float>((2 * Tp) * dm);
    p.ctc = d.ctc_vocab > 0 ? a.take<float>(M * (size_t)rs_ctc_pad(d.ctc_vocab)) : nullptr;
    return p;
}

size_t encoder_f32_workspace_bytes(const rs_ctx* ctx, int B, int t_max) {
    rs_arena a;
    plan_f32(ctx, B, t_max, a);
    return a.bytes() + ENC_F32_SLACK;
}

// The float32 encoder: the call sequence of rs_conformer_encoder_forward_impl (below) with float32 operands everywhere and no
// fusion that moves a rounding (there is none to move: nothing is rounded below float32).
int rs_encoder_forward_f32(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max, float* enc_out,
                           float* joint_enc, int32_t* enc_lens, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const rs_conformer& cf = *rs_conformer_of(ctx);
    const rs_f32_weights& w = cf.f32;
    rs_arena arena(workspace);
    const EncPlanF32 pl = plan_f32(ctx, B, t_max, arena);
    if (workspace_bytes < arena.bytes() + ENC_F32_SLACK)
        return rs_fail(ctx, RS_EWORKSPACE, "encoder (float32 mode): workspace %zu < %zu", workspace_bytes, arena.bytes() + ENC_F32_SLACK);
    int32_t* const lens_stage = pl.lens;
    float *const sa = pl.sa, *const sb = pl.sb, *const x = pl.x, *const hn = pl.hn, *const big = pl.big, *const ctxb = pl.ctxb, *const posp = pl.posp;
    const int C = d.sub_channels, dm = d.d_model, ff = d.ff_dim, S = d.sub_stages;
    const int Tp = pl.T[S], M = B * Tp;
    int rc;
#define RS_TRY(call) do { rc = (call); if (rc != RS_OK) return rc; } while (0)
    auto gemm = [&](const float* A, int lda, const float* W, int K, float* out, int ldc, int Mr, int N, int flags, const float* bias,
                    float alpha, const float* res) -> int {
        return rs_launch_gemm_f32(ctx, A, lda, W, K, out, ldc, Mr, N, K, flags, bias, alpha, res, nullptr, 0, 0, s);
    };
    // ---- subsampling
    RS_TRY(rs_launch_enc_lens(ctx, n_frames, B, lens_stage, s));
    if (Tp <= 0) return rs_fail(ctx, RS_EINVAL, "encoder (float32 mode): %d feature frames are too few for the subsampling", t_max);
    if (d.sub_kind == 1) {
        // ESPnet Conv2dSubsampling in float32: conv0 -> 3x3 patches -> the dense conv as one exact-f32 GEMM per chunk of utterances
        float* const col = pl.col;
        const int T1 = pl.T[1], F1 = pl.F[1], T2 = pl.T[2], F2 = pl.F[2];
        for (int b0 = 0; b0 < B; b0 += pl.chunk) {
            const int bc = B - b0 < pl.chunk ? B - b0 : pl.chunk;
            RS_TRY(rs_launch_sub2d_conv0_f32(ctx, feats, lens_stage, b0, bc, t_max, T1, F1, sa, s));
            RS_TRY(rs_launch_im2col3x3s2_f32(ctx, sa, bc, T1, F1, T2, F2, col, s));
            RS_TRY(rs_launch_gemm_f32(ctx, col, 9 * C, w.sub_conv1_w, 9 * C, sb + (size_t)b0 * T2 * F2 * C, C, bc * T2 * F2, C, 9 * C,
                                      RS_GEMM_BIAS | RS_GEMM_RELU | RS_GEMM_ROWMASK, cf.sub_conv1_b, 1.0f, nullptr,
                                      lens_stage + B + b0, F2, T2, s));
        }
    } else
    RS_TRY(rs_launch_sub_conv0_dw1_f32(ctx, feats, lens_stage, B, t_max, pl.T[2], pl.F[2], sa, s));
    for (int st = 2; st <= S && d.sub_kind == 0; ++st) {
        if (st > 2)
            RS_TRY(rs_launch_sub_dw_f32(ctx, sb, cf.sub_dw_w[st - 2], cf.sub_dw_b[st - 2], lens_stage + (st - 1) * B, B,
                                        pl.T[st - 1], pl.F[st - 1], pl.T[st], pl.F[st], sa, s));
        RS_TRY(rs_launch_gemm_f32(ctx, sa, C, w.sub_pw_w[st - 2], C, sb, C, B * pl.T[st] * pl.F[st], C, C,
                                  RS_GEMM_BIAS | RS_GEMM_RELU | RS_GEMM_ROWMASK, cf.sub_pw_b[st - 2], 1.0f, nullptr,
                                  lens_stage + (st - 1) * B, pl.F[st], pl.T[st], s));
    }
    {
        const int K = C * pl.F[S];
        RS_TRY(gemm(sb, K, w.sub_out_w, K, x, dm, M, dm, RS_GEMM_BIAS, cf.sub_out_b, d.xscaling ? sqrtf((float)dm) : 1.0f, nullptr));
    }
    const int32_t* lens = lens_stage + (S - 1) * B;
    RS_HIP(ctx, hipMemcpyAsync(enc_lens, lens, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (cf.tap_sub) RS_HIP(ctx, hipMemcpyAsync(cf.tap_sub, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));
    // ---- position rows for this T'
    const int tcap = (int)((w.pos_table_bytes / ((size_t)dm * 4) + 1) / 2);
    if (Tp > tcap) return rs_fail(ctx, RS_EINVAL, "encoder (float32 mode): T'=%d exceeds the registered pos.table.f32 capacity %d", Tp, tcap);
    const float* pos_slice = w.pos_table + (size_t)(tcap - Tp) * dm;
    const int npos = 2 * Tp - 1;
    const int RES = RS_GEMM_BIAS | RS_GEMM_RESIDUAL;
    for (int i = 0; i < d.n_layers; ++i) {
        const rs_layer_w& L = cf.layers[i];
        const rs_layer_w32& L32 = w.layers[i];
        // 1/2 FFN
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_ff1_g, L.ln_ff1_b, M, dm, d.ln_eps, nullptr, hn, s));
        RS_TRY(gemm(hn, dm, L32.ff1_w1, dm, big, ff, M, ff, RS_GEMM_BIAS | RS_GEMM_SILU, L.ff1_b1, 1.0f, nullptr));
        RS_TRY(gemm(big, ff, L32.ff1_w2, ff, x, dm, M, dm, RES, L.ff1_b2, 0.5f, x));
        // rel-pos MHSA
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_att_g, L.ln_att_b, M, dm, d.ln_eps, nullptr, hn, s));
        RS_TRY(gemm(hn, dm, L32.qkv_w, dm, big, 3 * dm, M, 3 * dm, RS_GEMM_BIAS, L.qkv_b, 1.0f, nullptr));
        RS_TRY(gemm(pos_slice, dm, L32.pos_w, dm, posp, dm, npos, dm, 0, nullptr, 1.0f, nullptr));
        RS_TRY(rs_launch_attention_f32(ctx, big, posp, L.bias_u, L.bias_v, lens, B, Tp, ctxb, s));
        RS_TRY(gemm(ctxb, dm, L32.out_w, dm, x, dm, M, dm, RES, L.out_b, 1.0f, x));
        // conv module (pw1 in NeMo's own row order: values | gates)
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_conv_g, L.ln_conv_b, M, dm, d.ln_eps, nullptr, hn, s));
        RS_TRY(gemm(hn, dm, L32.pw1_w, dm, big, 2 * dm, M, 2 * dm, RS_GEMM_BIAS, L32.pw1_b, 1.0f, nullptr));
        RS_TRY(rs_launch_glu_dwconv_f32(ctx, big, L.dw_w, L.dw_b, lens, B, Tp, dm, d.conv_kernel, ctxb, s));
        RS_TRY(gemm(ctxb, dm, L32.pw2_w, dm, x, dm, M, dm, RES, L.pw2_b, 1.0f, x));
        // 1/2 FFN
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_ff2_g, L.ln_ff2_b, M, dm, d.ln_eps, nullptr, hn, s));
        RS_TRY(gemm(hn, dm, L32.ff2_w1, dm, big, ff, M, ff, RS_GEMM_BIAS | RS_GEMM_SILU, L.ff2_b1, 1.0f, nullptr));
        RS_TRY(gemm(big, ff, L32.ff2_w2, ff, x, dm, M, dm, RES, L.ff2_b2, 0.5f, x));
        // output norm, in place (a wave holds its whole row in registers before it stores)
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_out_g, L.ln_out_b, M, dm, d.ln_eps, nullptr, x, s));
        for (size_t k = 0; k < cf.tap_ids.size(); ++k)
            if (cf.tap_ids[k] == i)
                RS_HIP(ctx, hipMemcpyAsync(cf.tap_layers + k * (size_t)M * dm, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));
    }
    // ESPnet: the encoder's after_norm on top of the last block's norm_final
    if (d.final_norm) RS_TRY(rs_launch_layernorm(ctx, x, cf.final_norm_g, cf.final_norm_b, M, dm, d.ln_eps, nullptr, x, s));
    if (enc_out) RS_HIP(ctx, hipMemcpyAsync(enc_out, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));
    RS_TRY(gemm(x, dm, w.jenc_w, dm, joint_enc, d.joint_hidden, M, d.joint_hidden, RS_GEMM_BIAS, ctx->jenc_b, 1.0f, nullptr));
    if (d.ctc_vocab > 0 && (cf.ctc_probs || cf.ctc_blank)) {
        const int Vp = rs_ctc_pad(d.ctc_vocab);
        float* z = cf.ctc_probs ? cf.ctc_probs : pl.ctc;
        RS_TRY(gemm(x, dm, w.ctc_w, dm, z, Vp, M, Vp, RS_GEMM_BIAS, cf.ctc_b, 1.0f, nullptr));
        RS_TRY(rs_launch_ctc_softmax(ctx, z, M, d.ctc_vocab, Vp, d.blank_id, cf.ctc_blank, s));
    }
#undef RS_TRY
    return RS_OK;
}

}  // namespace

// the encoder's share of rs_workspace_bytes
size_t rs_conformer_workspace_bytes_impl(const rs_ctx* ctx, int B, int t_max) {
    rs_arena measure;
    plan_encoder(ctx, B, t_max > 0 ? t_max : 1, measure);
    size_t enc = measure.bytes() + ENC_SLACK;
    if (ctx->has_f32) {                      // the float32 parity mode keeps float32 activations: about twice the scratch
        const size_t enc32 = encoder_f32_workspace_bytes(ctx, B, t_max > 0 ? t_max : 1);
        if (enc32 > enc) enc = enc32;
    }
    return enc;
}

int rs_conformer_encoder_forward_impl(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max, float* enc_out, float* joint_enc,
                                      int32_t* enc_lens, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (ctx->precision_f32)
        return rs_encoder_forward_f32(ctx, feats, n_frames, B, t_max, enc_out, joint_enc, enc_lens, workspace, workspace_bytes, s);
    const rs_dims& d = ctx->d;
    const rs_conformer& cf = *rs_conformer_of(ctx);
    rs_arena arena(workspace);
    const EncPlan pl = plan_encoder(ctx, B, t_max, arena);
    if (workspace_bytes < arena.bytes() + ENC_SLACK)
        return rs_fail(ctx, RS_EWORKSPACE, "encoder: workspace %zu < %zu", workspace_bytes, arena.bytes() + ENC_SLACK);
    int32_t* const lens_stage = pl.lens;
    uint16_t *const sa = pl.sa, *const sb = pl.sb, *const hn = pl.hn, *const big = pl.big, *const ctxb = pl.ctxb, *const posp = pl.posp;
    float *const x = pl.x, *const ln_stats = pl.stats;
    const int C = d.sub_channels, dm = d.d_model, ff = d.ff_dim, S = d.sub_stages;
    const int Tp = pl.T[S], M = B * Tp;
    int rc;
#define RS_TRY(call) do { rc = (call); if (rc != RS_OK) return rc; } while (0)

    // ---- subsampling -------------------------------------------------------------------------
    RS_TRY(rs_launch_enc_lens(ctx, n_frames, B, lens_stage, s));
    if (Tp <= 0) return rs_fail(ctx, RS_EINVAL, "encoder: %d feature frames are too few for the subsampling", t_max);
    if (d.sub_kind == 1) {
        // ESPnet Conv2dSubsampling: conv0 (VALU) -> 3x3 patches -> dense conv as one GEMM per chunk of utterances (bias, ReLU,
        // rows past an utterance's T2 zeroed), into sb [B][T2][F2][C]
        uint16_t* const col = pl.col;
        const int T1 = pl.T[1], F1 = pl.F[1], T2 = pl.T[2], F2 = pl.F[2];
        for (int b0 = 0; b0 < B; b0 += pl.chunk) {
            const int bc = B - b0 < pl.chunk ? B - b0 : pl.chunk;
            RS_TRY(rs_launch_sub2d_conv0(ctx, feats, lens_stage, b0, bc, t_max, T1, F1, sa, s));
            const bool patches_in_place = col == nullptr;                                   // (plan_encoder: $RS_SUB_IM2COL)
            if (!patches_in_place) RS_TRY(rs_launch_im2col3x3s2(ctx, sa, bc, T1, F1, T2, F2, col, s));
            rs_gemm_args g{};
            if (patches_in_place) { g.A = sa; g.conv_C = C; g.conv_T1 = T1; g.conv_F1 = F1; g.conv_T2 = T2; g.conv_F2 = F2; }
            else g.A = col;
            g.lda = 9 * C; g.W = cf.sub_conv1_w; g.ldw = 9 * C; g.out = sb + (size_t)b0 * T2 * F2 * C; g.ldc = C;
            g.M = bc * T2 * F2; g.N = C; g.K = 9 * C;
            g.flags = RS_GEMM_BIAS | RS_GEMM_RELU | RS_GEMM_ROWMASK; g.bias = cf.sub_conv1_b; g.alpha = 1.0f;
            g.mask_lens = lens_stage + B + b0; g.mask_rows_per_step = F2; g.mask_steps = T2;
            RS_TRY(rs_launch_gemm(ctx, g, s));
        }
    } else
    RS_TRY(rs_launch_sub_conv0_dw1(ctx, feats, lens_stage, B, t_max, pl.T[2], pl.F[2], sa, s));
    for (int st = 2; st <= S && d.sub_kind == 0; ++st) {
        if (st > 2)
            RS_TRY(rs_launch_sub_dw(ctx, sb, cf.sub_dw_w[st - 2], cf.sub_dw_b[st - 2], lens_stage + (st - 1) * B, st, B,
                                    pl.T[st - 1], pl.F[st - 1], pl.T[st], pl.F[st], sa, s));
        rs_gemm_args g{};
        g.A = sa; g.lda = C; g.W = cf.sub_pw_w[st - 2]; g.ldw = C; g.out = sb; g.ldc = C;
        g.M = B * pl.T[st] * pl.F[st]; g.N = C; g.K = C;
        g.flags = RS_GEMM_BIAS | RS_GEMM_RELU | RS_GEMM_ROWMASK; g.bias = cf.sub_pw_b[st - 2]; g.alpha = 1.0f;
        g.mask_lens = lens_stage + (st - 1) * B; g.mask_rows_per_step = pl.F[st]; g.mask_steps = pl.T[st];
        RS_TRY(rs_launch_gemm(ctx, g, s));
    }
    {
        rs_gemm_args g{};
        const int K = C * pl.F[S];
        g.A = sb; g.lda = K; g.W = cf.sub_out_w; g.ldw = K; g.out = x; g.ldc = dm; g.M = M; g.N = dm; g.K = K;
        g.flags = RS_GEMM_BIAS | RS_GEMM_OUT_F32; g.bias = cf.sub_out_b;
        g.alpha = d.xscaling ? sqrtf((float)dm) : 1.0f;
        RS_TRY(rs_launch_gemm(ctx, g, s));
    }
    const int32_t* lens = lens_stage + (S - 1) * B;
    RS_HIP(ctx, hipMemcpyAsync(enc_lens, lens, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (cf.tap_sub) RS_HIP(ctx, hipMemcpyAsync(cf.tap_sub, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));

    // ---- position table slice for this T ---------------------------------------------------------
    const int tcap = (int)((cf.pos_table_bytes / ((size_t)dm * 2) + 1) / 2);
    if (Tp > tcap) return rs_fail(ctx, RS_EINVAL, "encoder: T'=%d exceeds the registered pos.table capacity %d", Tp, tcap);
    const uint16_t* pos_slice = cf.pos_table + (size_t)(tcap - Tp) * dm;
    const int npos = 2 * Tp - 1;

    // res_ln: the residual operand still has to go through the PREVIOUS layer's output norm (deferred, see below)
    const rs_layer_w* res_ln = nullptr;
    auto gemm = [&](const uint16_t* A, int lda, const uint16_t* W, int K, void* out, int ldc, int Mr, int N, int flags,
                    const float* bias, float alpha, const float* res) -> int {
        rs_gemm_args g{};
        g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.out = out; g.ldc = ldc; g.M = Mr; g.N = N; g.K = K;
        g.flags = flags; g.bias = bias; g.alpha = alpha; g.residual = res;
        if (res && res_ln) { g.res_ln_stats = ln_stats; g.res_ln_g = res_ln->ln_out_g; g.res_ln_b = res_ln->ln_out_b; res_ln = nullptr; }
        return rs_launch_gemm(ctx, g, s);
    };
    const int RES = RS_GEMM_BIAS | RS_GEMM_RESIDUAL | RS_GEMM_OUT_F32;
    // fuse_glu (default 1): the GLU is applied to the float32 pw1 accumulators in the GEMM epilogue for EVERY batch
    // size — one rounding point, so an utterance's arithmetic does not depend on the batch it rides in
    const bool glu_fused = cf.fuse_glu != 0 && (dm % 32) == 0;

    for (int i = 0; i < d.n_layers; ++i) {
        const rs_layer_w& L = cf.layers[i];
        const bool last = i == d.n_layers - 1;
        // 1/2 FFN  (layers > 0: hn was produced by the previous layer's fused output-norm kernel)
        if (i == 0) RS_TRY(rs_launch_layernorm(ctx, x, L.ln_ff1_g, L.ln_ff1_b, M, dm, d.ln_eps, hn, nullptr, s));
        RS_TRY(gemm(hn, dm, L.ff1_w1, dm, big, ff, M, ff, RS_GEMM_BIAS | RS_GEMM_SILU, L.ff1_b1, 1.0f, nullptr));
        RS_TRY(gemm(big, ff, L.ff1_w2, ff, x, dm, M, dm, RES, L.ff1_b2, 0.5f, x));
        // rel-pos MHSA
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_att_g, L.ln_att_b, M, dm, d.ln_eps, hn, nullptr, s));
        RS_TRY(gemm(hn, dm, L.qkv_w, dm, big, 3 * dm, M, 3 * dm, RS_GEMM_BIAS, L.qkv_b, 1.0f, nullptr));
        const uint16_t* pproj = posp;
        if (L.pos_proj) pproj = L.pos_proj + (size_t)(tcap - Tp) * dm;      // rows of the pre-projected table
        else RS_TRY(gemm(pos_slice, dm, L.pos_w, dm, posp, dm, npos, dm, 0, nullptr, 1.0f, nullptr));
        RS_TRY(rs_launch_attention(ctx, big, pproj, L.bias_u, L.bias_v, lens, B, Tp, ctxb, s));
        RS_TRY(gemm(ctxb, dm, L.out_w, dm, x, dm, M, dm, RES, L.out_b, 1.0f, x));
        // conv module
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_conv_g, L.ln_conv_b, M, dm, d.ln_eps, hn, nullptr, s));
        // pw1's weight rows are interleaved (values / gates in blocks of 32): the GLU is applied in the GEMM
        // epilogue ([M][d] out, half the bytes written and read back); with fuse_glu = 0 the plain product is
        // stored and the conv kernel pairs the columns up itself
        if (glu_fused) {
            RS_TRY(gemm(hn, dm, L.pw1_w, dm, big, dm, M, 2 * dm, RS_GEMM_BIAS | RS_GEMM_GLU, L.pw1_b, 1.0f, nullptr));
            RS_TRY(rs_launch_glu_dwconv(ctx, big, RS_GLU_APPLIED, L.dw_w, L.dw_b, lens, B, Tp, dm, d.conv_kernel, ctxb, s));
        } else {
            RS_TRY(gemm(hn, dm, L.pw1_w, dm, big, 2 * dm, M, 2 * dm, RS_GEMM_BIAS, L.pw1_b, 1.0f, nullptr));
            RS_TRY(rs_launch_glu_dwconv(ctx, big, RS_GLU_BLOCK32, L.dw_w, L.dw_b, lens, B, Tp, dm, d.conv_kernel, ctxb, s));
        }
        RS_TRY(gemm(ctxb, dm, L.pw2_w, dm, x, dm, M, dm, RES, L.pw2_b, 1.0f, x));
        // 1/2 FFN
        RS_TRY(rs_launch_layernorm(ctx, x, L.ln_ff2_g, L.ln_ff2_b, M, dm, d.ln_eps, hn, nullptr, s));
        RS_TRY(gemm(hn, dm, L.ff2_w1, dm, big, ff, M, ff, RS_GEMM_BIAS | RS_GEMM_SILU, L.ff2_b1, 1.0f, nullptr));
        RS_TRY(gemm(big, ff, L.ff2_w2, ff, x, dm, M, dm, RES, L.ff2_b2, 0.5f, x));
        // output norm (in place on the residual stream; the last layer also emits the bf16 copy
        // that feeds the joint's encoder projection)
        if (last && d.final_norm) {
            // ESPnet: the block's norm_final, then the encoder's after_norm; hn = bf16 of the latter feeds the joint / CTC heads
            RS_TRY(rs_launch_layernorm(ctx, x, L.ln_out_g, L.ln_out_b, M, dm, d.ln_eps, nullptr, x, s));
        } else if (last) {
            // the f32 rows of the final norm are read by the caller's enc_out copy / a parity tap only
            bool want_f32 = enc_out != nullptr;
            for (size_t k = 0; k < cf.tap_ids.size(); ++k) want_f32 = want_f32 || cf.tap_ids[k] == i;
            RS_TRY(rs_launch_layernorm(ctx, x, L.ln_out_g, L.ln_out_b, M, dm, d.ln_eps, hn, want_f32 ? x : nullptr, s));
        } else {
            // output norm + the next layer's first norm on one read of the row.  The normalised f32 rows themselves have
            // ONE reader, the residual operand of the next layer's first FFN: unless a parity tap wants this layer's
            // output, they are not written (145 MB per boundary at B = 256) — the kernel leaves (mean, rstd) per row and
            // that GEMM's epilogue normalises x on the fly, with the same arithmetic (bit-identical: tests/test_gpu_pipeline.py)
            const rs_layer_w& Ln = cf.layers[i + 1];
            bool tapped = cf.defer_out_norm == 0;
            for (size_t k = 0; k < cf.tap_ids.size(); ++k) tapped = tapped || cf.tap_ids[k] == i;
            RS_TRY(rs_launch_layernorm2(ctx, x, L.ln_out_g, L.ln_out_b, Ln.ln_ff1_g, Ln.ln_ff1_b, M, dm, d.ln_eps,
                                        tapped ? x : nullptr, hn, tapped ? nullptr : ln_stats, s));
            if (!tapped) res_ln = &L;
        }
        for (size_t k = 0; k < cf.tap_ids.size(); ++k)     // parity taps: x now holds this layer's output
            if (cf.tap_ids[k] == i)
                RS_HIP(ctx, hipMemcpyAsync(cf.tap_layers + k * (size_t)M * dm, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));
    }
    if (d.final_norm) RS_TRY(rs_launch_layernorm(ctx, x, cf.final_norm_g, cf.final_norm_b, M, dm, d.ln_eps, hn, enc_out ? x : nullptr, s));
    if (enc_out) RS_HIP(ctx, hipMemcpyAsync(enc_out, x, (size_t)M * dm * 4, hipMemcpyDeviceToDevice, s));
    RS_TRY(gemm(hn, dm, ctx->jenc_w, dm, joint_enc, d.joint_hidden, M, d.joint_hidden, RS_GEMM_BIAS | RS_GEMM_OUT_F32,
                ctx->jenc_b, 1.0f, nullptr));
    if (d.ctc_vocab > 0 && (cf.ctc_probs || cf.ctc_blank)) {
        // CTC posteriors of every frame: logits by the same GEMM family, softmax in place
        float* z = cf.ctc_probs ? cf.ctc_probs : pl.ctc;
        const int Vp = rs_ctc_pad(d.ctc_vocab);
        RS_TRY(gemm(hn, dm, cf.ctc_w, dm, z, Vp, M, Vp, RS_GEMM_BIAS | RS_GEMM_OUT_F32, cf.ctc_b, 1.0f, nullptr));
        RS_TRY(rs_launch_ctc_softmax(ctx, z, M, d.ctc_vocab, Vp, d.blank_id, cf.ctc_blank, s));
    }
#undef RS_TRY
    return RS_OK;
}
