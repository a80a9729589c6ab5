// rs_common.h — internal declarations shared by the HIP translation units of librs_asr.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rs_asr.h"
#include "rs_arena.h"
#include "rs_family.h"
#include "rs_knobs.h"
#include "rs_tensors.h"

// ----------------------------------------------------------------------------------------
// device helpers
// ----------------------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned short u16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_to_f32(unsigned short v) {
    return __uint_as_float(((unsigned)v) << 16);
}
// round-to-nearest-even (same as torch .to(bfloat16)); lowers to v_cvt_pk_bf16_f32 on gfx950
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    return __builtin_bit_cast(unsigned short, (__bf16)f);
}
__device__ __forceinline__ u16x4_t pack_bf16x4(float a, float b, float c, float d) {
    const f32x4_t v = {a, b, c, d};
    return __builtin_bit_cast(u16x4_t, __builtin_convertvector(v, bf16x4_t));
}
__device__ __forceinline__ float round_bf16(float f) { return bf16_to_f32(f32_to_bf16(f)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// fast forms for the bf16 encoder path (v_exp_f32 + v_rcp_f32, ~1 ulp each; outputs are rounded to
// bf16 right after).  The exact-f32 decode path has its own polynomial versions in k_rnnt.hip.
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
// icefall's Swoosh activations (scaling.py; the Zipformer family): log(1 + exp(x - o)) - 0.08 x - c, softplus in its stable form
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.0f) + __logf(1.0f + __expf(-fabsf(x))); }
__device__ __forceinline__ float swoosh_l_f(float x) { return softplus_f(x - 4.0f) - 0.08f * x - 0.035f; }
__device__ __forceinline__ float swoosh_r_f(float x) { return softplus_f(x - 1.0f) - 0.08f * x - 0.313261687f; }
// the same in IEEE arithmetic (float32 parity mode): torch's F.softplus (log1p(exp(x)), identity above the threshold 20)
__device__ __forceinline__ float softplus_exact(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float swoosh_l_exact(float x) { return softplus_exact(x - 4.0f) - 0.08f * x - 0.035f; }
__device__ __forceinline__ float swoosh_r_exact(float x) { return softplus_exact(x - 1.0f) - 0.08f * x - 0.313261687f; }

// ----------------------------------------------------------------------------------------
// host side: context
// ----------------------------------------------------------------------------------------
struct rs_prof_launch { int32_t M, N, K, flags; double flops; float ms; };
struct rs_prof_slot {
    std::vector<hipEvent_t> ev;  // pairs (start, stop)
    std::vector<rs_prof_launch> detail;   // one record per bracketed launch since the last reset (shape tag + its time once read)
    size_t read = 0;             // records of `detail` whose events were already folded into ms_acc
    size_t used = 0;
    double flops = 0, bytes = 0;
    double ms_acc = 0;
    int64_t launches = 0;
};

struct rs_layer_w {
    const float *ln_ff1_g, *ln_ff1_b, *ln_att_g, *ln_att_b, *ln_conv_g, *ln_conv_b, *ln_ff2_g, *ln_ff2_b,
        *ln_out_g, *ln_out_b;
    const uint16_t *ff1_w1, *ff1_w2, *ff2_w1, *ff2_w2, *qkv_w, *out_w, *pos_w, *pw1_w, *pw2_w;
    const float *ff1_b1, *ff1_b2, *ff2_b1, *ff2_b2, *qkv_b, *out_b, *bias_u, *bias_v, *pw1_b, *pw2_b;
    const float *dw_w, *dw_b;
    const uint16_t* pos_proj;   // optional "L{i}.att.pos_proj": pos.table @ pos_w^T, bf16 [2*Tcap-1][d]; nullptr = project per call
};

// float32 parity mode (k_f32.hip): the dense weights once more, unrounded.  Norm weights, biases, depthwise taps and
// the attention position biases are float32 in the throughput mode already and are shared.
struct rs_layer_w32 {
    const float *ff1_w1, *ff1_w2, *ff2_w1, *ff2_w2, *qkv_w, *out_w, *pos_w, *pw1_w, *pw2_w;
    const float* pw1_b;         // pointwise_conv1 bias in NeMo's own row order (values | gates); the bf16 copy is interleaved
};
struct rs_f32_weights {
    const float* sub_pw_w[4] = {};
    const float* sub_conv1_w = nullptr;  // ESPnet family: "sub.conv1.w.f32" [C][9C]
    const float* ctc_w = nullptr;        // ESPnet family: "ctc.w.f32" [ctc rows padded to 4][d]
    const float* sub_out_w = nullptr;
    std::vector<rs_layer_w32> layers;
    const float* jenc_w = nullptr;
    const float* pos_table = nullptr;   // "pos.table.f32": f32 [2*Tcap-1][d]
    size_t pos_table_bytes = 0;
};

// A family's own state: resolved weights, dimensions, taps.  The context owns exactly one, made by its create function.
struct rs_family_state { virtual ~rs_family_state() = default; };

// The Conformer family (rs_create: NeMo and ESPnet, told apart by rs_dims.frontend_kind / sub_kind / final_norm / ctc_vocab);
// filled by k_conformer.hip.  The Zipformer family's rs_k2 lives in k_zipformer.hip, the AV-HuBERT family's rs_avsr in k_avsr.hip.
struct rs_conformer : rs_family_state {
    int head_dim = 0, sub_freq = 0;
    const float *sub_conv0_w = nullptr, *sub_conv0_b = nullptr;
    const float *sub_dw_w[4] = {}, *sub_dw_b[4] = {};
    const uint16_t* sub_pw_w[4] = {};
    const float* sub_pw_b[4] = {};
    const uint16_t* sub_out_w = nullptr;
    const float* sub_out_b = nullptr;
    std::vector<rs_layer_w> layers;
    const float *fe_mvn_mean = nullptr, *fe_mvn_istd = nullptr;
    const uint16_t* sub_conv1_w = nullptr;
    const float* sub_conv1_b = nullptr;
    const float *final_norm_g = nullptr, *final_norm_b = nullptr;
    const uint16_t* ctc_w = nullptr;
    const float* ctc_b = nullptr;
    float *ctc_probs = nullptr, *ctc_blank = nullptr;     // rs_encoder_set_ctc_out
    const uint16_t* pos_table = nullptr;                  // "pos.table": bf16 [2*Tcap-1][d]
    size_t pos_table_bytes = 0;
    rs_f32_weights f32;
    // parity taps (rs_encoder_set_taps): copies of the residual stream taken inside rs_encoder_forward
    float* tap_sub = nullptr;
    float* tap_layers = nullptr;
    std::vector<int> tap_ids;
    // options (rs_set_option)
    int defer_out_norm = 1;         // 1 = a layer's output norm is applied by the next layer's first residual GEMM (f32 rows not stored); bit-identical to 0
    int fuse_glu = 1;               // conv module: 1 = GLU in the pw1 GEMM epilogue (every batch size: one rounding point, batch-invariant);
                                    // 0 = plain pw1 product, GLU in the depthwise kernel ($RS_FUSE_GLU; the layout tests set the option)
};
struct rs_k2;
struct rs_avsr;

struct rs_ctx {
    int device = 0;
    rs_family family = RS_FAM_CONFORMER;            // set once by rs_create / rs_k2_create / rs_avsr_create
    std::unique_ptr<rs_family_state> state;         // that family's own state: read through rs_conformer_of / rs_k2_of / rs_avsr_of
    rs_dims d{};
    bool finalized = false;
    std::string err;
    rs_tensor_table tensors;        // rs_set_tensor: name -> (pointer, bytes); read through rs_weights (below) by every rs_finalize
    // front-end tables
    const float *fe_window = nullptr, *fe_fb_w = nullptr, *fe_twiddle = nullptr;
    const int32_t* fe_fb_idx = nullptr;
    // decoder and joint
    const uint16_t* jenc_w = nullptr;
    const float* jenc_b = nullptr;
    const float* lstm_w4[8] = {};   // optional "pred.lstm{l}.w4": fragment-major with rows permuted to (unit group, gate, unit)
    const float* k2_conv_w = nullptr;   // stateless decoder: grouped Conv1d over the last two tokens, f32 [D][4][2]
    const float *embed = nullptr, *lstm_w[8] = {}, *lstm_b[8] = {}, *jpred_w = nullptr, *jpred_b = nullptr,
                *jout_w = nullptr, *jout_b = nullptr;
    // screened joint (optional tensors joint.out.w16 / .wrm / .bpad / .wmax; k_rnnt.hip)
    const uint16_t* jout_w16 = nullptr;
    const float *jout_wrm = nullptr, *jout_bpad = nullptr, *jout_wmax = nullptr;
    // options (rs_set_option)
    bool decode_screen = true;
    bool decode_narrow = true;      // narrow-tile LSTM / projection kernels (k_rnnt.hip)
    bool gemm_f32_x3 = false;       // rs_launch_gemm_f32 / rs_launch_conv3x3_f32 multiply with three bf16 terms per float32 product (k_f32.hip X3)
    int k2_conv2_fused = -1;        // conv2 with its patches gathered into LDS: -1 = the table's RS_K2_CONV2_FUSED (default 1); rs_set_option("k2_conv2_fused")
    int k2_cnx_fused = -1;          // ConvNeXt pointwise pair as one kernel: -1 = the table's RS_K2_CNX_FUSED (default 1); rs_set_option("k2_cnx_fused")
    int n_cus = 0;                  // compute units of the device (rs_n_cus: queried on first use)
    bool has_f32 = false;           // the "*.f32" tensors of the float32 parity mode are registered (all or none)
    int precision_f32 = 0;          // rs_set_option("precision_f32"): 1 = rs_encoder_forward runs the float32 encoder
    bool has_i8 = false;            // at least one quantized Linear ("<name>.i8") is registered
    int precision_i8 = 0;           // rs_set_option("precision_i8"): the float32 encoder with its quantized Linears ("*.i8") on k_int8.hip
    bool env_read = false;          // the table's context defaults were applied (once, by the first rs_finalize; rs_set_option wins afterwards)
    // k_gemm_bf16.hip, register-resident weight form ($RS_GEMM_BREG): fragment-major copies of registered GEMM weights (made on first
    // use, owned by the context) and a scratch for operands that are not registered tensors (re-shuffled on every launch)
    std::unordered_map<const void*, void*> wfm;
    void* wfm_scratch = nullptr;
    size_t wfm_scratch_bytes = 0;
    // profiling
    int prof_mask = 0;
    rs_prof_slot prof[8];
    int32_t prof_tag[4] = {0, 0, 0, 0};   // (M, N, K, flags) of the launch about to be bracketed (set by the GEMM launcher)
};

// A context's family state as its own type; nullptr for a context of another family (and for a null context).
inline rs_conformer* rs_conformer_of(const rs_ctx* ctx) {
    return ctx && ctx->family == RS_FAM_CONFORMER ? static_cast<rs_conformer*>(ctx->state.get()) : nullptr;
}
rs_k2* rs_k2_of(const rs_ctx* ctx);       // k_zipformer.hip
rs_avsr* rs_avsr_of(const rs_ctx* ctx);   // k_avsr.hip

// Opt-in for more than 64 KiB of dynamic LDS, once per (device, kernel): the attribute is per device and the
// first launch of a kernel can come from any thread (the decode worker and the encoder thread both start
// kernels), so the bookkeeping is a mutex-guarded set keyed by the context's device — not a function-local flag.
int rs_ensure_dynamic_lds(rs_ctx* ctx, const void* func, int bytes);

int rs_fail(rs_ctx* ctx, int code, const char* fmt, ...);

// The family guard (rs_family.h), first statement of every exported function that takes a context.  RS_GUARD returns the refusal's
// code with its text in the context; RS_GUARD_QUERY is for the size and frame-count queries, which return `zero` and write nothing.
inline int rs_guard(rs_ctx* ctx, rs_entry e) {
    char msg[512];
    const int rc = rs_family_guard(e, ctx != nullptr, ctx ? ctx->family : RS_FAM_CONFORMER, ctx && ctx->finalized, msg, sizeof msg);
    if (rc != RS_OK && ctx) ctx->err = msg;
    return rc;
}
inline bool rs_guard_query(const rs_ctx* ctx, rs_entry e) {
    return rs_family_guard(e, ctx != nullptr, ctx ? ctx->family : RS_FAM_CONFORMER, ctx && ctx->finalized, nullptr, 0) == RS_OK;
}
#define RS_GUARD(ctx, entry) do { if (const int _g = rs_guard((ctx), RS_ENTRY_##entry); _g != RS_OK) return _g; } while (0)
#define RS_GUARD_QUERY(ctx, entry, zero) do { if (!rs_guard_query((ctx), RS_ENTRY_##entry)) return zero; } while (0)

// The registered tensors as typed pointers (rs_tensors.h's sticky reader): the first failing get() is kept, every later one does
// nothing and leaves its output alone; a finalize calls fail() where it needs the pointers to be good.
struct rs_weights : rs_tensor_reader {
    explicit rs_weights(const rs_ctx* ctx) : rs_tensor_reader(ctx->tensors) {}
    template <typename T>
    void get(const std::string& name, size_t elems, const T*& out) {
        const void* p = out;
        get_bytes(name, elems * sizeof(T), p);
        out = static_cast<const T*>(p);
    }
    int fail(rs_ctx* ctx) const { return rs_fail(ctx, rc, "%s", msg.c_str()); }
};
// the screened joint's optional operands "joint.out.w16" / ".wrm" / ".bpad" / ".wmax" -> ctx->jout_*: all four or none (rs_api.hip)
void rs_get_screened_joint(rs_ctx* ctx, rs_weights& r);
// compute units of the context's device (256 when the query fails), cached in ctx->n_cus
int rs_n_cus(rs_ctx* ctx);

#define RS_HIP(ctx, call)                                                              \
    do {                                                                               \
        hipError_t _e = (call);                                                        \
        if (_e != hipSuccess)                                                          \
            return rs_fail((ctx), RS_EHIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call, \
                           hipGetErrorString(_e));                                     \
    } while (0)

#define RS_CHECK_LAUNCH(ctx, what)                                                            \
    do {                                                                                      \
        hipError_t _e = hipGetLastError();                                                    \
        if (_e != hipSuccess)                                                                 \
            return rs_fail((ctx), RS_EHIP, "launch %s failed: %s", (what), hipGetErrorString(_e)); \
    } while (0)

// Profiling bracket around the kernel launches of one class: rs_prof_begin records the start event and the class's bookkeeping,
// rs_prof_end the stop event.  Launchers do not call the two themselves; they open an rs_prof_scope, which ends the bracket
// exactly once on every way out of its block (RS_HIP, RS_CHECK_LAUNCH and every other early return included).  The stop event
// belongs right after the bracket's last launch: call end() there, or close the scope's block there, when more follows.
int rs_prof_class_index(int klass);
void rs_prof_begin(rs_ctx* ctx, int klass, hipStream_t s, double flops, double bytes);
void rs_prof_end(rs_ctx* ctx, int klass, hipStream_t s);
struct rs_prof_scope {
    rs_prof_scope(rs_ctx* ctx, int klass, hipStream_t s, double flops, double bytes) : ctx(ctx), klass(klass), s(s) { rs_prof_begin(ctx, klass, s, flops, bytes); }
    rs_prof_scope(const rs_prof_scope&) = delete;
    rs_prof_scope& operator=(const rs_prof_scope&) = delete;
    ~rs_prof_scope() { end(); }
    void end() { if (open) rs_prof_end(ctx, klass, s); open = false; }
private:
    rs_ctx* ctx; int klass; hipStream_t s; bool open = true;
};

// ----------------------------------------------------------------------------------------
// kernel launchers (one per .hip file); all return RS_OK / RS_E*
// ----------------------------------------------------------------------------------------
struct rs_gemm_args {
    const uint16_t* A; int lda;
    const uint16_t* W; int ldw;
    void* out; int ldc;
    int M, N, K, flags;
    const float* bias; float alpha;
    const float* residual;
    const int32_t* mask_lens; int mask_rows_per_step; int mask_steps;
    // residual = LayerNorm(residual operand; res_ln_g, res_ln_b) with per-row (mean, rstd) in res_ln_stats [M][2]
    // (nullptr: the residual operand is used as it is)
    const float* res_ln_stats; const float* res_ln_g; const float* res_ln_b;
    // residual GEMMs only: also store the result rounded to bf16 at out_bf16[m * ld_bf16 + n] (the A operand of the next GEMM:
    // the Zipformer family has no norm between a residual add and the next Linear, so the copy would otherwise be a pass of its own)
    uint16_t* out_bf16; int ld_bf16;
    // conv_C > 0: A is not a matrix but the channels-last input [Bc][conv_T1][conv_F1][conv_C] of a 3 x 3, stride-2, un-padded
    // convolution; row m = (b * conv_T2 + t2) * conv_F2 + f2 of the product is the patch of output pixel (t2, f2), K = 9 * conv_C
    // ordered (kernel row, kernel column, channel) — the matrix im2col3x3s2 would write, read in place: a kernel row of a patch
    // is 3 * conv_C contiguous elements of the input (lda is ignored; plain bf16 output with the row mask only)
    int conv_C, conv_T1, conv_F1, conv_T2, conv_F2;
};
int rs_launch_gemm(rs_ctx* ctx, const rs_gemm_args& a, hipStream_t s);
int rs_launch_layernorm(rs_ctx* ctx, const float* x, const float* g, const float* b, int M, int d, float eps,
                        uint16_t* out_bf16, float* out_f32, hipStream_t s);
// out_f32 == nullptr: the first norm's rows are not stored; `stats` [M][2] receives its (mean, rstd) per row instead
int rs_launch_layernorm2(rs_ctx* ctx, const float* x, const float* g1, const float* b1, const float* g2, const float* b2,
                         int M, int d, float eps, float* out_f32, uint16_t* out_bf16, float* stats, hipStream_t s);
int rs_launch_attention(rs_ctx* ctx, const uint16_t* qkv, const uint16_t* pos, const float* bias_u,
                        const float* bias_v, const int32_t* lens, int B, int T, uint16_t* out, hipStream_t s);
int rs_launch_glu_dwconv(rs_ctx* ctx, const uint16_t* x, int layout, const float* w, const float* b, const int32_t* lens,
                         int B, int T, int d, int k, uint16_t* out, hipStream_t s);
int rs_launch_frontend(rs_ctx* ctx, const float* audio, const int32_t* lens, int B, int audio_stride,
                       int pad_left, int pad_right, int t_max, float* feats, int32_t* n_frames, float* raw,
                       hipStream_t s);
int rs_launch_sub_conv0_dw1(rs_ctx* ctx, const float* feats, const int32_t* lens_stage, int B, int t_max, int T2,
                            int F2, uint16_t* out, hipStream_t s);
int rs_launch_sub_dw(rs_ctx* ctx, const uint16_t* in, const float* w, const float* b, const int32_t* lens_out,
                     int stage, int B, int t_in, int f_in, int t_out, int f_out, uint16_t* out, hipStream_t s);
// float32 parity mode (k_f32.hip, k_subsample.hip)
int rs_launch_gemm_f32(rs_ctx* ctx, const float* A, int lda, const float* W, int ldw, float* out, int ldc, int M, int N, int K,
                       int flags, const float* bias, float alpha, const float* residual, const int32_t* mask_lens,
                       int mask_rows_per_step, int mask_steps, hipStream_t s);
// the same product for M <= 128 rows (a decoder step's hypothesis rows): N / 16 workgroups, K cut over the four waves (k_f32.hip)
int rs_launch_conv3x3_f32(rs_ctx* ctx, const float* in, int n_img, int H, int Wd, int C, int OH, int OW, int stride, const float* W, int Cout,
                          const float* bn_scale, const float* bn_shift, const float* residual, const float* prelu, float* out, int one_by_one, hipStream_t s);
int rs_launch_gemm_f32_skinny(rs_ctx* ctx, const float* A, int lda, const float* W, int ldw, float* out, int ldc, int M, int N, int K, int flags,
                              const float* bias, const float* residual, hipStream_t s);
int rs_launch_attention_f32(rs_ctx* ctx, const float* qkv, const float* pos, const float* bias_u, const float* bias_v,
                            const int32_t* lens, int B, int T, float* out, hipStream_t s);
int rs_launch_glu_dwconv_f32(rs_ctx* ctx, const float* x, const float* w, const float* b, const int32_t* lens, int B, int T,
                             int d, int k, float* out, hipStream_t s);
// int8 mode (k_int8.hip): (sx, zx) per group of `group` rows from the first lens[g] rows, columns < K -> qp f32 [n_groups][2]; then
// out = epilogue(float(sum_k (xq - zx)(Wq - zw)) * fl(sx sw) + bias) with W int8 [N][ldw], colsum[n] = sum_{k < K} W[n][k], wq = (sw, zw)
int rs_launch_i8_range(rs_ctx* ctx, const float* A, int lda, const int32_t* lens, int group, int n_groups, int K, float* qp, hipStream_t s);
int rs_launch_gemm_i8q(rs_ctx* ctx, const float* A, int lda, int group, const float* qp, const int8_t* W, int ldw, const int32_t* colsum,
                       const float* wq, float* out, int ldc, int M, int N, int K, int flags, const float* bias, const float* residual, hipStream_t s);
int rs_launch_sub_conv0_dw1_f32(rs_ctx* ctx, const float* feats, const int32_t* lens_stage, int B, int t_max, int T2, int F2,
                                float* out, hipStream_t s);
int rs_launch_sub_dw_f32(rs_ctx* ctx, const float* in, const float* w, const float* b, const int32_t* lens_out, int B, int t_in,
                         int f_in, int t_out, int f_out, float* out, hipStream_t s);
int rs_launch_enc_lens(rs_ctx* ctx, const int32_t* n_frames, int B, int32_t* lens_out, hipStream_t s);
// ESPnet family (k_espnet.hip)
int rs_launch_sub2d_conv0(rs_ctx* ctx, const float* feats, const int32_t* lens1, int b0, int Bc, int t_max, int T1, int F1,
                          uint16_t* out, hipStream_t s);
int rs_launch_im2col3x3s2(rs_ctx* ctx, const uint16_t* in, int Bc, int T1, int F1, int T2, int F2, uint16_t* out, hipStream_t s);
int rs_launch_ctc_softmax(rs_ctx* ctx, float* logits, int M, int V, int ld, int blank, float* blank_out, hipStream_t s);
int rs_launch_sub2d_conv0_f32(rs_ctx* ctx, const float* feats, const int32_t* lens1, int b0, int Bc, int t_max, int T1, int F1,
                              float* out, hipStream_t s);
int rs_launch_im2col3x3s2_f32(rs_ctx* ctx, const float* in, int Bc, int T1, int F1, int T2, int F2, float* out, hipStream_t s);
// rows of the registered CTC head ("ctc.w" / "ctc.b") and row pitch of the posteriors: the vocabulary padded to a multiple of 4
static inline int rs_ctc_pad(int v) { return (v + 3) / 4 * 4; }
// the families' parts of the shared entry points (k_conformer.hip, k_zipformer.hip, k_avsr.hip)
int rs_conformer_finalize_impl(rs_ctx* ctx);
size_t rs_conformer_workspace_bytes_impl(const rs_ctx* ctx, int B, int t_max);
int rs_conformer_encoder_forward_impl(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max, float* enc_out, float* joint_enc,
                                      int32_t* enc_lens, void* workspace, size_t workspace_bytes, hipStream_t s);
int rs_avsr_finalize_impl(rs_ctx* ctx);
const rs_avsr_dims* rs_avsr_dims_of(const rs_ctx* ctx);   // k_avsr.hip: nullptr unless an avsr context
int rs_k2_finalize_impl(rs_ctx* ctx);
int rs_k2_unk_id(const rs_ctx* ctx);
size_t rs_k2_workspace_bytes_impl(const rs_ctx* ctx, int B, int t_max);
int rs_k2_enc_frames_impl(const rs_ctx* ctx, int n_feat);
int rs_k2_encoder_forward_impl(rs_ctx* ctx, const float* feats, const int32_t* n_frames, int B, int t_max, float* enc_out, float* joint_enc,
                               int32_t* enc_lens, void* workspace, size_t workspace_bytes, hipStream_t s);
// depthwise Conv1d over time with a compile-time kernel size (7 / 15 / 31), frame mask, bias, activation (0 SiLU, 1 SwooshR):
// x bf16 [B*T][d] -> out bf16 [B*T][d]; d % 64 == 0 (k_layernorm.hip)
int rs_launch_dwconv_act(rs_ctx* ctx, const uint16_t* x, const float* w, const float* b, const int32_t* lens, int B, int T, int d, int k,
                         int act, uint16_t* out, hipStream_t s);
// output length of one subsampling conv (k 3, s 2): padding 1 (NeMo dw_striding) or none (ESPnet Conv2dSubsampling)
static inline int rs_conv_len(int n, int sub_kind) { return sub_kind ? (n >= 3 ? (n - 3) / 2 + 1 : 0) : (n > 0 ? (n + 2 - 3) / 2 + 1 : 0); }
