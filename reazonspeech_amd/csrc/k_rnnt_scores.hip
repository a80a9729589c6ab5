// k_rnnt_scores.hip — token log-probabilities of a finished transducer search (rs_rnnt_token_scores): a teacher-forced pass over
// the search's own output.  It runs AFTER any of the searches (greedy, ALSD, the default beam search, the modified beam search)
// and touches none of their kernels, workspaces or results.
//
// For token u of utterance b, emitted at frame t:
//     logp[b][u] = z[id] - lse(z),   z = W_out . act(f[b][t] + g(y_<u)) + b_out      (the model's own distribution: no blank
//                                                                                      penalty, no hotword bonus)
//     top1[b][u] = argmax_v z[v], the lowest index on ties (a greedy result: top1 == ids)
// g(y_<u) is the prediction network's output after the start context and the first u labels.  Every number is float32 in the
// fixed order of the searches, restated by tests/token_scores_checker.c, which the results equal bit for bit:
//   g       LSTM families: u_cap lock-step steps over the B rows through the search's own launcher (rs_rnnt_launch_lstm_pred:
//           the rows with u < n_ids[b] are the work list, the vector of step u is written straight into the log g_log[u][b][:]);
//           Zipformer family: the stateless decoder has no chain — one decoder launch per chunk over its (b, u) rows with their
//           two context tokens ([-1, blank] at u = 0)
//   z       rnnt_tile_kernel<4> (k_rnnt.hip, the exact tile over rows a_pre[r] = act(f + g), as the modified beam search runs it):
//           the K-slice order of rs_oracle_joint_argmax
//   lse     m = max_{v < V} z[v]; lane l of the row's wave adds rs_expf(z[v] - m) for v = l, l + 64, .. in increasing v from 0; the
//           64 partials are folded by p[l] = p[l] + p[l + off], off = 32, 16, .., 1 (rs_oracle_lse, oracle/rnnt_alsd.c); then
//           z[id] - (m + rs_logf(p[0])).  The logits row is padded to a multiple of 64 columns; only v < V is read.
// The (b, u) pairs with u < n_ids[b] form one compacted row list in (b, u) order; it is scored in chunks of R rows (R a multiple
// of 32 that follows from the workspace given: the logits of a chunk are R x 64 ceil(V / 64) floats), so a row's bits depend
// neither on the chunk size nor on what else is in the batch.
// THESE GPUS ARE SHARED: frames are checked against enc_lens (and tp_max) and ids against V before they index anything; a bad
// entry is replaced by frame 0 / the blank for the loads, its slot gets NaN and the call returns RS_EINVAL after the sync.
// rs_rnnt_token_scores_rows: B text rows, row b scored against the frames of utterance row_utt[b] (-1: the row has no tokens and
// none of its slots is touched).  row_utt is checked by the plan before anything indexes with it (rs_align_rows_plan.h); only the
// joint-encoder frames and enc_lens are read through it, so a row's bits are those of rs_rnnt_token_scores on replicated frames.
// Compiled with -ffp-contract=off.
#include "k_rnnt_common.h"
#include "rs_align_rows_plan.h"

namespace {

struct ScoreArgs {
    const int32_t* enc_lens;   // [B]
    const int32_t* ids;        // [B][u_cap]
    const int32_t* frames;     // [B][u_cap] frame of each token (steps = 1: alignment step = frame + index)
    const int32_t* n_ids;      // [B]
    int B, u_cap, tp_max, V, blank, steps;                  // B: the text rows (rs_rnnt_token_scores: one per utterance)
    const int32_t* row_utt;    // [B] rs_rnnt_token_scores_rows: the utterance of row b (nullptr: row b is utterance b)
    int n_utt;
    // workspace
    int32_t* n_ok;             // [B] n_ids clamped to 0..u_cap
    int32_t* row_b;            // [B * u_cap] utterance of compacted row w
    int32_t* row_u;            // [B * u_cap] token index of compacted row w
    int32_t* info;             // [0] rows in all, [1] longest count, [2] a bad entry was met, [3] what row_utt does wrong (RS_ROWS_*)
};

__device__ __forceinline__ bool id_ok(const ScoreArgs& a, int id) { return id >= 0 && id < a.V; }
// frame of token (b, u), or -1 when it is outside the utterance
__device__ __forceinline__ int frame_of(const ScoreArgs& a, int b, int u) {
    int t = a.frames[(size_t)b * a.u_cap + u];
    if (a.steps) t -= u;
    int T = a.enc_lens[a.row_utt ? a.row_utt[b] : b];       // (checked by the plan)
    T = T < a.tp_max ? T : a.tp_max;
    return (t >= 0 && t < T) ? t : -1;
}

// ---- the compacted row list, in (b, u) order.  One workgroup of 256 threads: thread i owns a contiguous run of utterances. ----
__global__ __launch_bounds__(256) void scores_plan_kernel(ScoreArgs a) {
    __shared__ int part[256];
    __shared__ int longest_s, bad_s, err_s;
    const int tid = threadIdx.x;
    if (tid == 0) { longest_s = 0; bad_s = 0; err_s = 0; }
    __syncthreads();
    const int per = (a.B + 255) / 256;
    const int b0 = tid * per, b1 = (b0 + per) < a.B ? (b0 + per) : a.B;
    if (a.row_utt) {                                        // nothing indexes with row_utt before every entry passed
        int err = 0;
        for (int b = b0; b < b1; ++b) err |= rs_align_rows_check_row(a.row_utt, a.n_utt, b);
        if (err) atomicOr(&err_s, err);
        __syncthreads();
        if (err_s) {
            if (tid == 0) { a.info[0] = 0; a.info[1] = 0; a.info[2] = 0; a.info[3] = err_s; }
            return;
        }
    }
    int sum = 0, longest = 0, bad = 0;
    for (int b = b0; b < b1; ++b) {
        int n = (a.row_utt && a.row_utt[b] == -1) ? 0 : a.n_ids[b];    // a skipped row has no tokens
        if (n < 0 || n > a.u_cap) { bad = 1; n = n < 0 ? 0 : a.u_cap; }
        a.n_ok[b] = n;
        sum += n;
        longest = n > longest ? n : longest;
    }
    part[tid] = sum;
    if (longest) atomicMax(&longest_s, longest);
    if (bad) atomicOr(&bad_s, 1);
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        a.info[0] = run; a.info[1] = longest_s; a.info[2] = bad_s; a.info[3] = 0;
    }
    __syncthreads();
    int w = part[tid];
    for (int b = b0; b < b1; ++b) {
        const int n = a.n_ok[b];
        for (int u = 0; u < n; ++u, ++w) { a.row_b[w] = b; a.row_u[w] = u; }
    }
}

// ---- LSTM families, step u of the chain: the rows with u < n_ids[b] take their previous label (the blank at u = 0) ----
__global__ __launch_bounds__(256) void scores_lstm_step_kernel(ScoreArgs a, DecodeState st, int u) {
    __shared__ int n_act_s;
    if (threadIdx.x == 0) n_act_s = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < a.B; b += 256) {
        if (u >= a.n_ok[b]) continue;
        int tok = a.blank;
        if (u > 0) {
            tok = a.ids[(size_t)b * a.u_cap + u - 1];
            if (!id_ok(a, tok)) tok = a.blank;            // (its own slot gets NaN from the pick kernel)
        }
        st.token[b] = tok;
        st.act[atomicAdd(&n_act_s, 1)] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) st.counters[0] = n_act_s;
}

// ---- Zipformer family, chunk rows w0 .. w0 + n: decoder row r takes the two tokens before token u of its utterance ----
__global__ __launch_bounds__(256) void scores_k2_context_kernel(ScoreArgs a, DecodeState st, int w0, int n) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) st.counters[0] = n;
    if (r >= n) return;
    const int b = a.row_b[w0 + r], u = a.row_u[w0 + r];
    int t1 = u >= 1 ? a.ids[(size_t)b * a.u_cap + u - 1] : a.blank;
    int t0 = u >= 2 ? a.ids[(size_t)b * a.u_cap + u - 2] : (u == 1 ? a.blank : -1);
    if (u >= 1 && !id_ok(a, t1)) t1 = a.blank;
    if (u >= 2 && !id_ok(a, t0)) t0 = a.blank;
    st.token2[r] = t0; st.token[r] = t1; st.act[r] = r;
}

// ---- a_pre[r] = act(f[b][t] + g) of the chunk's rows, and the tile kernel's row list (the identity) ----
// g_log != nullptr: row (b, u)'s vector is g_log[u][b][:] (LSTM families); else st.g[r][:] (this chunk's decoder launch)
__global__ __launch_bounds__(256) void scores_gather_kernel(ScoreArgs a, DecodeState st, const float* __restrict__ f,
                                                            const float* __restrict__ g_log, float* __restrict__ a_pre, int J,
                                                            int w0, int n, int list_pitch, int parity) {
    const int j4 = J / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * j4) return;
    const int r = (int)(i / j4), k = (int)(i - (long long)r * j4) * 4;
    const int b = a.row_b[w0 + r], u = a.row_u[w0 + r];
    int t = frame_of(a, b, u);
    if (t < 0) t = 0;                                     // tp_max >= 1: row 0 exists
    const int fb = a.row_utt ? a.row_utt[b] : b;
    const float4 fv = *reinterpret_cast<const float4*>(f + ((size_t)fb * a.tp_max + t) * J + k);
    const float* gr = g_log ? g_log + ((size_t)u * a.B + b) * J : st.g + (size_t)r * J;
    const float4 gv = *reinterpret_cast<const float4*>(gr + k);
    *reinterpret_cast<float4*>(a_pre + (size_t)r * J + k) = rs_joint_act4(fv, gv, st.joint_act);
    if (k == 0) st.alive[(size_t)parity * list_pitch + r] = r;
    if (i == 0) st.counters[2 + parity] = n;
}

// ---- log-softmax pick: one wave per row of the chunk ----
__global__ __launch_bounds__(256) void rnnt_logp_pick_kernel(ScoreArgs a, const float* __restrict__ z, int zstride, int w0, int n,
                                                             float* __restrict__ logp, int32_t* __restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int b = a.row_b[w0 + r], u = a.row_u[w0 + r];
    const size_t slot = (size_t)b * a.u_cap + u;
    const int id = a.ids[slot];
    if (frame_of(a, b, u) < 0 || !id_ok(a, id)) {
        if (lane == 0) {
            logp[slot] = __uint_as_float(0x7fc00000u);
            if (top1) top1[slot] = -1;
            a.info[2] = 1;
        }
        return;
    }
    const float* zr = z + (size_t)r * zstride;
    const int V = a.V;
    // max and argmax (lowest index on ties): each lane scans its columns in increasing v, then a butterfly
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = zr[v];
        if (x > m) { m = x; mi = v; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(m, off, 64);
        const int oi = __shfl_xor(mi, off, 64);
        if (ov > m || (ov == m && oi < mi)) { m = ov; mi = oi; }
    }
    // lane-strided sums over v < V only, then the 32 -> 1 tree: after the step `off`, lanes l < off hold p[l] + p[l + off]
    float p = 0.0f;
    for (int v = lane; v < V; v += 64) p = p + rs_expf(zr[v] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p = p + __shfl_down(p, off, 64);
    if (lane == 0) {
        logp[slot] = zr[id] - (m + rs_logf(p));
        if (top1) top1[slot] = mi;
    }
}

// ---- workspace ----
struct ScoreLayout {
    DecodeState st{};
    ScoreArgs a{};
    float* g_log = nullptr;    // LSTM families: [u_cap][B][J]
    float* a_pre = nullptr;    // [R][J]
};

// R = rows per chunk (a multiple of 32)
void scores_layout(const rs_ctx* ctx, int B, int u_cap, size_t R, rs_arena& ar, ScoreLayout& l) {
    const rs_dims& d = ctx->d;
    const size_t H = d.pred_hidden, J = d.joint_hidden, rows = (size_t)B * u_cap;
    DecodeState& st = l.st;
    l.a.n_ok = ar.take<int32_t>(B);
    l.a.row_b = ar.take<int32_t>(rows);
    l.a.row_u = ar.take<int32_t>(rows);
    l.a.info = ar.take<int32_t>(16);
    st.counters = ar.take<int32_t>(16);
    if (ctx->k2_conv_w) {          // the decoder runs over the chunk's rows; the projection's state commit copies h_tmp / c_tmp to h / c
        st.h_tmp = ar.take<float>(R * H); st.c_tmp = st.h_tmp;
        st.h = ar.take<float>(R * H); st.c = st.h;
        st.g = ar.take<float>(R * J);
        st.token = ar.take<int32_t>(R); st.token2 = ar.take<int32_t>(R); st.act = ar.take<int32_t>(R);
    } else {                       // the chain runs over the B utterances (h and c adjacent: one memset clears both)
        const size_t state = (size_t)d.pred_layers * B * H;
        st.h = ar.take<float>(state); st.c = ar.take<float>(state);
        st.h_tmp = ar.take<float>(state); st.c_tmp = ar.take<float>(state);
        st.token = ar.take<int32_t>(B); st.act = ar.take<int32_t>(B);
        l.g_log = ar.take<float>(rows * J);
        st.g = l.g_log;
    }
    st.alive = ar.take<int32_t>(2 * R);                                      // [2][R]: the tile kernel reads list (chunk & 1) at pitch R
    l.a_pre = ar.take<float>(R * J);
    st.zapprox = ar.take<float>(R * (size_t)rs_joint_zstride(d));
    st.a_pre = l.a_pre;
    st.joint_act = d.joint_act;
}
constexpr size_t SCORES_MAX_R = 32 * 65535;                // the tile kernel's grid

size_t scores_bytes(const rs_ctx* ctx, int B, int u_cap, size_t R) {
    rs_arena ar;
    ScoreLayout l;
    scores_layout(ctx, B, u_cap, R, ar, l);
    return ar.bytes() + RS_DECODE_SLACK;
}

}  // namespace

size_t rs_rnnt_token_scores_workspace_bytes_impl(const rs_ctx* ctx, int B, int u_cap) { return scores_bytes(ctx, B, u_cap, 32); }

// rows per chunk that `workspace_bytes` holds (0: below the minimum), at most the rows there can be
size_t rs_rnnt_token_scores_chunk_rows(const rs_ctx* ctx, int B, int u_cap, size_t workspace_bytes) {
    const size_t least = scores_bytes(ctx, B, u_cap, 32);
    if (workspace_bytes < least) return 0;
    const size_t per32 = scores_bytes(ctx, B, u_cap, 64) - least;
    size_t most = ((size_t)B * u_cap + 31) / 32 * 32;
    if (most < 32) most = 32;
    if (most > SCORES_MAX_R) most = SCORES_MAX_R;
    size_t R = 32 + 32 * ((workspace_bytes - least) / per32);
    if (R > most) R = most;
    while (R > 32 && scores_bytes(ctx, B, u_cap, R) > workspace_bytes) R -= 32;
    return R;
}

// B text rows; row_utt == nullptr: rs_rnnt_token_scores (row b is utterance b), else rs_rnnt_token_scores_rows over n_utt utterances
static int scores_run(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int n_utt, int tp_max, const int32_t* row_utt,
                      int B, const int32_t* ids, const int32_t* frames, const int32_t* n_ids, int u_cap, int steps, float* logp,
                      int32_t* top1, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const int L = d.pred_layers, H = d.pred_hidden, J = d.joint_hidden, V = d.n_logits;
    const bool k2 = ctx->k2_conv_w != nullptr;
    if (int rc = rs_rnnt_check_dims(ctx, "token scores"); rc != RS_OK) return rc;
    if (k2 && L != 1) return rs_fail(ctx, RS_EINVAL, "token scores: unsupported prediction network");
    if ((long long)B * u_cap > 0x3fffffffLL) return rs_fail(ctx, RS_EINVAL, "token scores: B x u_cap too large");
    const size_t R = rs_rnnt_token_scores_chunk_rows(ctx, B, u_cap, workspace_bytes);
    if (R == 0)
        return rs_fail(ctx, RS_EINVAL, "token scores: workspace %zu < %zu", workspace_bytes, rs_rnnt_token_scores_workspace_bytes_impl(ctx, B, u_cap));
    rs_arena arena(workspace);
    ScoreLayout l;
    scores_layout(ctx, B, u_cap, R, arena, l);
    DecodeState& st = l.st;
    ScoreArgs& a = l.a;
    a.enc_lens = enc_lens; a.ids = ids; a.frames = frames; a.n_ids = n_ids;
    a.B = B; a.u_cap = u_cap; a.tp_max = tp_max; a.V = V; a.blank = d.blank_id; a.steps = steps;
    a.row_utt = row_utt; a.n_utt = n_utt;
    if (k2) st.unk = rs_k2_unk_id(ctx);
    const int zstride = rs_joint_zstride(d);

    rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
    int32_t info[4] = {0, 0, 0, 0};
    hipLaunchKernelGGL(scores_plan_kernel, dim3(1), dim3(256), 0, s, a);
    RS_HIP(ctx, hipMemcpyAsync(info, a.info, sizeof info, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    if (row_utt && info[3])
        return rs_fail(ctx, RS_EINVAL, "token scores: row_utt %s (nothing was scored)",
                       (info[3] & RS_ROWS_BAD_UTT) ? "names an utterance outside 0..B-1 (-1 skips a row)"
                       : (info[3] & RS_ROWS_DECREASE) ? "decreases" : "gives one utterance more rows than RS_ALIGN_ROWS_PER_UTT_MAX");
    const int n_rows = info[0], longest = info[1];
    if (n_rows < 0 || (long long)n_rows > (long long)B * u_cap || longest < 0 || longest > u_cap)
        return rs_fail(ctx, RS_ESTATE, "token scores: inconsistent plan");

    if (!k2 && n_rows > 0) {
        const size_t state_bytes = (size_t)L * B * H * 4;
        RS_HIP(ctx, hipMemsetAsync(st.h, 0, 2 * rs_align(state_bytes), s));
        for (int u = 0; u < longest; ++u) {
            DecodeState su = st;
            su.g = l.g_log + (size_t)u * B * J;           // the projection writes row b of step u's slab
            hipLaunchKernelGGL(scores_lstm_step_kernel, dim3(1), dim3(256), 0, s, a, su, u);
            if (int rc = rs_rnnt_launch_lstm_pred(ctx, &su, B, s); rc != RS_OK) return rc;
        }
    }
    int chunk = 0;
    for (int w0 = 0; w0 < n_rows; w0 += (int)R, ++chunk) {
        const int n = n_rows - w0 < (int)R ? n_rows - w0 : (int)R;
        if (k2) {
            hipLaunchKernelGGL(scores_k2_context_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, st, w0, n);
            if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st, n, s); rc != RS_OK) return rc;
        }
        const long long n_thr = (long long)n * (J / 4);
        hipLaunchKernelGGL(scores_gather_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s, a, st, joint_enc,
                           (const float*)(k2 ? nullptr : l.g_log), l.a_pre, J, w0, n, (int)R, chunk & 1);
        if (int rc = rs_rnnt_launch_joint_logits_indirect(ctx, &st, joint_enc, (int)R, n, tp_max, 1, chunk, s); rc != RS_OK) return rc;
        hipLaunchKernelGGL(rnnt_logp_pick_kernel, dim3((n + 3) / 4), dim3(256), 0, s, a, st.zapprox, zstride, w0, n, logp, top1);
    }
    RS_CHECK_LAUNCH(ctx, "token scores");
    RS_HIP(ctx, hipMemcpyAsync(info, a.info, sizeof info, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    prof.end();
    if (info[2]) return rs_fail(ctx, RS_EINVAL, "token scores: a count outside 0..u_cap, a frame outside its utterance or an id outside the vocabulary (its slot is NaN)");
    return RS_OK;
}

int rs_rnnt_token_scores_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                              const int32_t* frames, const int32_t* n_ids, int u_cap, int steps, float* logp, int32_t* top1,
                              void* workspace, size_t workspace_bytes, hipStream_t s) {
    return scores_run(ctx, joint_enc, enc_lens, B, tp_max, nullptr, B, ids, frames, n_ids, u_cap, steps, logp, top1, workspace,
                      workspace_bytes, s);
}

int rs_rnnt_token_scores_rows_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max,
                                   const int32_t* row_utt, int R, const int32_t* ids, const int32_t* frames, const int32_t* n_ids,
                                   int u_cap, int steps, float* logp, int32_t* top1, void* workspace, size_t workspace_bytes,
                                   hipStream_t s) {
    return scores_run(ctx, joint_enc, enc_lens, B, tp_max, row_utt, R, ids, frames, n_ids, u_cap, steps, logp, top1, workspace,
                      workspace_bytes, s);
}
