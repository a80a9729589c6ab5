// k_rnnt_mbs.hip — sherpa-onnx's modified_beam_search for the Zipformer family (stateless decoder + tanh joiner), the second
// decoding method of sherpa_onnx.OfflineRecognizer.from_transducer, which K2Model stands for (reference call site:
// pkg/k2-asr/src/huggingface.py:73-83; the reference passes greedy_search, `decoding_method="modified_beam_search"` with
// `max_active_paths` is the constructor's other offline transducer method).
//
// [UPSTREAM, not vendored, PARITY UNPINNED like the greedy search] OfflineTransducerModifiedBeamSearchDecoder::Decode without
// LM, Hypotheses::Add, GetMostProbable(length_norm = true); hotwords (ContextGraph) and the n-gram LM follow below.  The
// algorithm, as built here:
//   * per utterance one starting hypothesis ys = [-1, blank] (context_size = 2 entries), log_prob = 0, no timestamps;
//   * for every encoder frame t < enc_lens[b], with H <= K live hypotheses (K = max_active_paths):
//       1. dec[h] = decoder_proj(decoder(last two tokens of h))                   (k2_decoder_kernel + rnnt_pred16_kernel)
//       2. logits[h][:] = output_linear(tanh(f[b][t] + dec[h])); blank_penalty > 0: logits[h][blank] -= blank_penalty
//       3. lp[h][v] = ((logits[h][v] - max_h) - log(sum_h)) + log_prob[h]
//       4. the K largest of the H x V values, flat index c = h V + v;  EQUAL VALUES: THE LOWER FLAT INDEX FIRST
//       5. in that order: copy hypothesis h; v neither blank nor <unk>: append v to ys and t to the timestamps;
//          log_prob = lp[h][v]; add to the new set — a hypothesis whose ys equals one already in the set (compared in full:
//          length and every token) is merged into it: log_prob = logaddexp(old, new), the tokens / timestamps of the one
//          added FIRST stay;
//   * result: the hypothesis with the largest log_prob / len(ys) (len counts the 2 context entries; without
//     RS_MBS_LENGTH_NORM the largest log_prob);  EQUAL FINAL SCORES: THE HYPOTHESIS THAT ENTERED THE LAST SET FIRST.
// Upstream leaves both orders in capitals open (a partial sort, an unordered map) and keeps log_prob in double; here every
// number is float32 in one order, restated by tests/k2_mbs_checker.c, which the results equal bit for bit:
//   log-softmax of a row: thread i of 256 owns the columns v = i + 256 q.  max: any order (exact).  sum: s_i = the chain over
//   q ascending of s = s + rs_expf(x - max), from 0; inside each wave of 64 the butterfly s_l = s_l + s_(l xor off) for
//   off = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits), then ((w0 + w1) + w2) + w3 over the four waves.
//   merge: rs_logaddexpf(old, new) of k_rnnt_common.h.  final score: log_prob / (float)len(ys).
//
// The batch advances in lock step over the frames; hypothesis rows are r = utterance * K + slot.  One frame = 5 launches,
// none of them waits for the host (the whole search is enqueued once, one synchronisation at the end):
//   mbs_act_kernel      a_pre[r] = tanh(f[b][t] + g[dec[r]]) for the live rows (a blank extension keeps its parent's decoder
//                       row by index: K decoder rows per utterance, a label extension takes a free one)
//   rnnt_tile_kernel<4> exact f32 joint logits [rows][V] on v_mfma_f32_16x16x4_f32 -> zbuf (k_rnnt.hip, same K-slice order as
//                       rs_oracle_joint_argmax)
//   mbs_select_kernel   a workgroup per utterance: steps 3 - 5 and, at the utterance's last frame, the result
//   k2_decoder_kernel + rnnt_pred16_kernel over the decoder rows that took a label
// Utterances past their length are on no list and their workgroups return at once.
//
// HOTWORDS (rs_rnnt_mbs_hotwords).  [UPSTREAM, not vendored, PARITY UNPINNED] sherpa-onnx's ContextGraph — Build, FillFailOutput,
// ForwardOneStep(strict_mode = false), Finalize — as OfflineTransducerModifiedBeamSearchDecoder::Decode uses it; the graph and
// the step are stated in include/rs_asr.h.  In the search: every hypothesis row carries a node index (MbsState.ctx, ping-pong
// like the records; the starting hypothesis carries its graph's root).  Step 4 is untouched — the K best are selected on values
// WITHOUT any bonus.  In step 5, before the merge, each of the at most 8 candidates that appends a label v walks the graph once:
// (delta, state') = step(parent's state, v), log_prob = lp[h][v] + delta; one that appends nothing keeps its parent's state.  The
// merge adds log_probs with their bonuses inside; tokens, timestamps AND state of the entry added first stay.  At the utterance's
// last frame every entry of the new set gets log_prob = log_prob + (-node_score[state]) (Finalize) BEFORE the winner is chosen;
// scores[b] is the winner's log_prob after that.  Float32 order of one step, restated by tests/k2_mbs_checker.c:
//   child hit:  score = token_score[n];       otherwise:  score = node_score[n] - node_score[state]
//   non-strict exit (output_score[n] != 0):  delta = (score + out) - node_score[n];     otherwise:  delta = score + output_score[n]
// It is the hotword form of mbs_select_kernel (template parameter HW): no further launch, no host round trip.  The plain
// instantiations are the ones launched when no utterance of the call has a graph; inside the hotword form a workgroup whose
// utterance has none takes the plain statements.
// The graph is read-only flat arrays (rs_hotwords), all graphs of the call concatenated.  A root can have thousands of children:
// a child is found by bisection of the node's sorted token list (every lane of wave 0 computes the same value; no lane scans
// a list).  THESE GPUS ARE SHARED, so the walk cannot spin or read out of bounds whatever the table holds: every loop is
// counted (a fail step strictly lowers the level in a valid table, so max_level + 1 fail steps suffice and that is the bound;
// a bisection halves an interval of < 2^31 entries, 32 steps), and a node or child index outside the table is replaced by the root
// before it is used — a corrupt table can give a wrong bonus, nothing else.  rs_hotwords_check (rs_api.hip) refuses such tables
// on the host before upload.  The walk itself (hw_root, hw_node, hw_child, hw_step) is k_rnnt_hotwords.h.
//
// N-GRAM LM (rs_rnnt_mbs_lm; the table and `step` are stated in include/rs_asr.h, the walk is k_rnnt_ngram.h, shared with ALSD).
// [UPSTREAM, not vendored, UNVERIFIED] the slot is believed to be icefall's modified_beam_search_lm_shallow_fusion: the LM term is
// added to a candidate AFTER the top-K pick, not inside it (ALSD's LM form ranks with it, on purpose: see the header).  Every
// hypothesis row carries an LM state (MbsState.lmctx, ping-pong; the starting hypothesis stands at `start`).  Step 4 is untouched.
// In step 5, before the merge, a selected candidate that appends a label v: lp = lp[h][v]; with a graph lp = lp + delta;
// (l, s') = step(s, v); log_prob = lp + (alpha * l), the product rounded first; state s'.  One that appends nothing keeps score and
// state and makes no walk.  The merge keeps the first entry's LM state too; Finalize applies to the LM-inclusive score; no
// end-of-sentence term.  An LM walk usually backs off through every level (a hotword walk usually ends at its first node), so the at
// most 8 walks of a frame do not run one after another on all lanes: lane j < n_cand of wave 0 computes candidate j whole — hotword
// step if the utterance has a graph, LM step, score — and the three results are broadcast by __shfl, so everything below (merge,
// decoder rows, winner) stays uniform.  What this saves over one lane doing all walks has not been measured.  The LM form is the
// template parameter LM of mbs_init_kernel / mbs_select_kernel; it is compiled with HW on and carries the call's graphs or none
// (graph_of == nullptr: every utterance takes the no-graph statements).  The plain and hotword instantiations are the same text
// without the `if constexpr (LM)` statements and are the ones launched when the call has no model (lm == NULL, no nodes, alpha 0).
// Compiled with -ffp-contract=off.
#include "k_rnnt_common.h"
#include "k_rnnt_hotwords.h"
#include "k_rnnt_ngram.h"

#include <type_traits>


namespace {

constexpr int MBS_MAX_K = 8;      // max_active_paths
constexpr int MBS_THREADS = 256;  // of the selection kernel: 4 waves
constexpr int MBS_CONTEXT = 2;    // context_size of the stateless decoder (k2_decoder_kernel reads two tokens)

struct MbsState {
    // hypothesis records, [2] = ping-pong: frame t reads set (t & 1) and writes set ((t + 1) & 1)
    int32_t* len[2];     // [rows] tokens after the context
    float* score[2];     // [rows] log_prob
    int32_t* last0[2];   // [rows] token before last (context included)
    int32_t* last1[2];   // [rows] last token
    int32_t* dec[2];     // [rows] decoder row of the hypothesis, 0..K-1 inside its utterance
    int32_t* y[2];       // [rows][cap] tokens
    int32_t* fr[2];      // [rows][cap] frame of each token
    int32_t* n_hyp[2];   // [B]
    int32_t* ctx[2];     // [rows] hotwords: node of the context graph the hypothesis stands at (nullptr without hotwords)
    int32_t* lmctx[2];   // [rows] n-gram LM: the LM state of the hypothesis (nullptr without an LM)
    int cap;
};

// the graphs of a call and the walk over them: k_rnnt_hotwords.h (shared with the ALSD search)
using MbsNoHw = RnntNoHw;
using MbsHw = RnntHw;
struct MbsHwLm : MbsHw { // n-gram LM: the model and its weight next to the graphs, which may be absent (graph_of == nullptr)
    rs_ngram lm;
    float alpha;
};
template <bool HW, bool LM>
using MbsArg = std::conditional_t<LM, MbsHwLm, std::conditional_t<HW, MbsHw, MbsNoHw>>;
// root of utterance b's graph; the LM form may carry no graphs at all
template <bool LM, class A>
__device__ __forceinline__ int mbs_root(const A& hw, int b) {
    if constexpr (LM) { if (hw.graph_of == nullptr) return -1; }
    return hw_root(hw, b);
}

template <bool HW, bool LM = false>
__global__ void mbs_init_kernel(DecodeState st, MbsState ms, const int32_t* __restrict__ enc_lens, int B, int K, int blank,
                                int32_t* __restrict__ n_ids, float* __restrict__ scores, MbsArg<HW, LM> hw) {
    // single workgroup: the starting hypothesis of every utterance, its decoder row and the first work lists
    __shared__ int n_alive_s;
    if (threadIdx.x == 0) n_alive_s = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int row = b * K;
        ms.len[0][row] = 0; ms.score[0][row] = 0.0f; ms.last0[0][row] = -1; ms.last1[0][row] = blank; ms.dec[0][row] = 0;
        ms.n_hyp[0][b] = 1;
        if constexpr (HW) { const int r = mbs_root<LM>(hw, b); ms.ctx[0][row] = r < 0 ? 0 : r; }
        if constexpr (LM) ms.lmctx[0][row] = lm_node(hw.lm, hw.lm.start);
        st.token2[row] = -1; st.token[row] = blank; st.act[b] = row;
        if (n_ids != nullptr) { n_ids[b] = 0; scores[b] = 0.0f; }   // the result of an utterance without frames (rs_rnnt_mbs_nbest: the caller clears its lists)
        if (enc_lens[b] > 0) st.alive[atomicAdd(&n_alive_s, 1)] = row;
    }
    __syncthreads();
    // counters: [0] decoder rows to compute, [1] overflow flag, [2],[3] live rows of list 0 / 1
    if (threadIdx.x == 0) { st.counters[0] = B; st.counters[1] = 0; st.counters[2] = n_alive_s; st.counters[3] = 0; }
}

// a_pre[row] = act(f[utt][t] + g[utt * K + dec[row]]) for the rows of list (t & 1); one thread per 4 elements
__global__ __launch_bounds__(256) void mbs_act_kernel(DecodeState st, MbsState ms, const float* __restrict__ f, float* __restrict__ a_pre,
                                                      int rows, int Tp, int J, int K, int t) {
    const int list = t & 1;
    const int n = st.counters[2 + list];
    const int q4 = J / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)n * q4; i += (long long)gridDim.x * 256) {
        const int idx = (int)(i / q4), q = (int)(i - (long long)idx * q4);
        const int row = st.alive[(size_t)list * rows + idx];
        const int utt = row / K;
        const int drow = utt * K + ms.dec[list][row];
        const float4 a = reinterpret_cast<const float4*>(f + ((size_t)utt * Tp + t) * J)[q];
        const float4 g = reinterpret_cast<const float4*>(st.g + (size_t)drow * J)[q];
        reinterpret_cast<float4*>(a_pre + (size_t)row * J)[q] = rs_joint_act4(a, g, st.joint_act);
    }
}

// NVR > 0: V <= 256 NVR and a hypothesis's logits row is read ONCE into NVR registers per thread, every load in flight before the
// first comparison; maximum, exp-sum and the running top-K then walk the registers.  NVR = 0: any V, three passes over memory,
// the same arithmetic in the same order.
// HW: the hotword form; LM: the n-gram form (HW on as well).  The other forms are the same text without the `if constexpr` statements.
// nbest == 0: the one result, as ever (ids / frames [B][out_cap], n_ids / scores [B]).  nbest >= 1 (rs_rnnt_mbs_nbest; a uniform
// run-time branch at the utterance's last frame, no further launch): the entries of the last set ranked by the winner's rule applied
// down the list — the greatest norm first, of equal norms the one that entered the set first — into ids / frames
// [B][nbest][out_cap], n_ids / scores / norm_scores [B][nbest], n_hyps [B].
template <int NVR, bool HW, bool LM = false>
__global__ __launch_bounds__(MBS_THREADS) void mbs_select_kernel(
    DecodeState st, MbsState ms, const float* __restrict__ zbuf, int zstride, const int32_t* __restrict__ enc_lens, int rows, int K,
    int V, int blank, int unk, int t, float blank_penalty, int length_norm, int out_cap, int32_t* __restrict__ ids,
    int32_t* __restrict__ frames, int32_t* __restrict__ n_ids, float* __restrict__ scores, int nbest, float* __restrict__ norm_scores,
    int32_t* __restrict__ n_hyps, MbsArg<HW, LM> hw) {
    static_assert(HW || !LM, "the LM form is compiled with the hotword statements");
    const int b = blockIdx.x;
    const int T = enc_lens[b];
    if (t >= T) return;                                   // skipped, not masked
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = t & 1, pn = p ^ 1;
    const int H = ms.n_hyp[p][b];
    const int cap = ms.cap;

    __shared__ float s_max[MBS_MAX_K][4], s_sum[MBS_MAX_K][4];
    __shared__ float s_cz[MBS_MAX_K][4];
    __shared__ int s_cv[MBS_MAX_K][4];
    __shared__ float s_val[MBS_MAX_K];                    // the K best (value, flat index), descending
    __shared__ int s_idx[MBS_MAX_K];
    __shared__ int s_prow[MBS_MAX_K], s_tok[MBS_MAX_K], s_dec[MBS_MAX_K];   // the new set, in the order of entry
    __shared__ float s_score[MBS_MAX_K];
    __shared__ int s_nnew;
    __shared__ int s_ctx[HW ? MBS_MAX_K : 1];             // hotwords: the context state of each entry of the new set
    int root = -1;                                        // hotwords: the root of the utterance's graph, -1 = it has none
    if constexpr (HW) root = mbs_root<LM>(hw, b);
    __shared__ int s_lm[LM ? MBS_MAX_K : 1];              // n-gram LM: the LM state of each entry of the new set

    // ---- steps 3 + 4a: every thread's K best of its own columns over all H rows (sorted: value desc, flat index asc; a thread
    // meets its flat indices in ascending order, so a later equal value never displaces an earlier one) ----
    float tz[MBS_MAX_K];
    int tv[MBS_MAX_K];
#pragma unroll
    for (int k = 0; k < MBS_MAX_K; ++k) { tz[k] = -INFINITY; tv[k] = -1; }
    float thr = -INFINITY;                                // value of the thread's K-th entry once its list is full
    bool full = false;
    for (int h = 0; h < H; ++h) {
        const int row = b * K + h;
        const float* zr = zbuf + (size_t)row * zstride;
        const float hs = ms.score[p][row];
        auto logit = [&](int v) {
            float x = zr[v];
            if (v == blank && blank_penalty > 0.0f) x = x - blank_penalty;
            return x;
        };
        float zreg[NVR > 0 ? NVR : 1];
        float m = -INFINITY;
        if constexpr (NVR > 0) {
#pragma unroll
            for (int q = 0; q < NVR; ++q) {
                const int v = tid + MBS_THREADS * q;
                zreg[q] = zr[v < V ? v : V - 1];
            }
#pragma unroll
            for (int q = 0; q < NVR; ++q) {
                const int v = tid + MBS_THREADS * q;
                if (v == blank && blank_penalty > 0.0f) zreg[q] = zreg[q] - blank_penalty;
                if (v < V && zreg[q] > m) m = zreg[q];
            }
        } else {
            for (int v = tid; v < V; v += MBS_THREADS) { const float x = logit(v); if (x > m) m = x; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(m, off, 64); if (o > m) m = o; }
        if (lane == 0) s_max[h][wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(s_max[h][0], s_max[h][1]), fmaxf(s_max[h][2], s_max[h][3]));
        float sum = 0.0f;
        if constexpr (NVR > 0) {
#pragma unroll
            for (int q = 0; q < NVR; ++q)
                if (tid + MBS_THREADS * q < V) sum = sum + rs_expf(zreg[q] - m);
        } else {
            for (int v = tid; v < V; v += MBS_THREADS) sum = sum + rs_expf(logit(v) - m);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
        if (lane == 0) s_sum[h][wave] = sum;
        __syncthreads();
        const float lg = rs_logf(((s_sum[h][0] + s_sum[h][1]) + s_sum[h][2]) + s_sum[h][3]);
        auto offer = [&](int v, float x) {
            const float lp = ((x - m) - lg) + hs;
            if (full && !(lp > thr)) return;
            float cz = lp;
            int cv = h * V + v;
            bool ins = false;                             // once placed, everything behind shifts down one slot
#pragma unroll
            for (int k = 0; k < MBS_MAX_K; ++k) {
                if (k < K && (ins || tv[k] < 0 || cz > tz[k])) {
                    const float sz = tz[k]; const int sv = tv[k];
                    tz[k] = cz; tv[k] = cv;
                    cz = sz; cv = sv;
                    ins = true;
                }
                if (k == K - 1) { thr = tz[k]; full = tv[k] >= 0; }
            }
        };
        if constexpr (NVR > 0) {
#pragma unroll
            for (int q = 0; q < NVR; ++q) {
                const int v = tid + MBS_THREADS * q;
                if (v < V) offer(v, zreg[q]);
            }
        } else {
            for (int v = tid; v < V; v += MBS_THREADS) offer(v, logit(v));
        }
    }

    // ---- step 4b: the K best of the workgroup: K rounds, each pops the best list head (wave butterfly, then the 4 waves) ----
    int n_cand = K;
    for (int j = 0; j < K; ++j) {
        float bz = tz[0];
        int bv = tv[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float oz = __shfl_xor(bz, off, 64);
            const int ov = __shfl_xor(bv, off, 64);
            if (rs_before(oz, ov, bz, bv)) { bz = oz; bv = ov; }
        }
        if (lane == 0) { s_cz[j][wave] = bz; s_cv[j][wave] = bv; }
        __syncthreads();
        bz = s_cz[j][0]; bv = s_cv[j][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (rs_before(s_cz[j][w], s_cv[j][w], bz, bv)) { bz = s_cz[j][w]; bv = s_cv[j][w]; }
        if (bv < 0) { n_cand = j; break; }                // fewer than K values exist (H V < K); uniform over the workgroup
        if (tid == 0) { s_val[j] = bz; s_idx[j] = bv; }
        if (tv[0] == bv) {                                // the owner pops its head
#pragma unroll
            for (int k = 0; k + 1 < MBS_MAX_K; ++k) { tz[k] = tz[k + 1]; tv[k] = tv[k + 1]; }
            tz[MBS_MAX_K - 1] = -INFINITY; tv[MBS_MAX_K - 1] = -1;
        }
    }
    __syncthreads();

    // ---- step 5 (wave 0, every lane computes the same values): expansion, merging, decoder rows, the result ----
    if (wave == 0) {
        int cprow[MBS_MAX_K], ctok[MBS_MAX_K], cplen[MBS_MAX_K];
        float csc[MBS_MAX_K];
        const int32_t* cy[MBS_MAX_K];
        unsigned dup = 0;
#pragma unroll
        for (int j = 0; j < MBS_MAX_K; ++j) {
            cprow[j] = b * K; ctok[j] = -1; cplen[j] = 0; csc[j] = 0.0f; cy[j] = ms.y[p];
            if (j < n_cand) {
                const int c = s_idx[j];
                const int h = c / V, v = c - h * V;
                ctok[j] = (v != blank && v != unk) ? v : -1;
                cprow[j] = b * K + h;
                cplen[j] = ms.len[p][cprow[j]];
                cy[j] = ms.y[p] + (size_t)cprow[j] * cap;
                csc[j] = s_val[j];
            }
        }
        // hotwords: one walk per candidate that appends a label, before the merge; the others keep their parent's state
        int cctx[HW ? MBS_MAX_K : 1];
        [[maybe_unused]] int clm[LM ? MBS_MAX_K : 1];
        if constexpr (LM) {
            // n-gram LM: an LM walk usually backs off through every level, so the walks run side by side: lane j computes candidate j
            // whole — the hotword step if the utterance has a graph, the LM step, the score — and the three results are broadcast
            float msc = 0.0f;
            int mctx = 0, mlm = 0;
            if (lane < n_cand) {
                const int c = s_idx[lane];
                const int h = c / V, v = c - h * V;
                const int prow = b * K + h;
                msc = s_val[lane];
                if (root >= 0) mctx = ms.ctx[p][prow];
                mlm = ms.lmctx[p][prow];
                if (v != blank && v != unk) {
                    if (root >= 0) {
                        int nx = root;
                        const float delta = hw_step(hw.g, root, mctx, v, &nx);
                        msc = msc + delta;
                        mctx = nx;
                    }
                    int ln = 0;
                    const float l = lm_step(hw.lm, mlm, v, &ln);
                    msc = msc + (hw.alpha * l);
                    mlm = ln;
                }
            }
#pragma unroll
            for (int j = 0; j < MBS_MAX_K; ++j) {
                const float bsc = __shfl(msc, j, 64);
                cctx[j] = __shfl(mctx, j, 64);
                clm[j] = __shfl(mlm, j, 64);
                if (j < n_cand) csc[j] = bsc;
            }
        } else if constexpr (HW) {
#pragma unroll
            for (int j = 0; j < MBS_MAX_K; ++j) {
                cctx[j] = 0;
                if (j < n_cand && root >= 0) {
                    cctx[j] = ms.ctx[p][cprow[j]];
                    if (ctok[j] >= 0) {
                        int nx = root;
                        const float delta = hw_step(hw.g, root, cctx[j], ctok[j], &nx);
                        csc[j] = csc[j] + delta;
                        cctx[j] = nx;
                    }
                }
            }
        }
        // a candidate whose token sequence equals that of an earlier entry adds its probability to it
#pragma unroll
        for (int j = 1; j < MBS_MAX_K; ++j) {
            if (j >= n_cand) continue;
            bool merged = false;
            const int n = cplen[j] + (ctok[j] >= 0 ? 1 : 0);
#pragma unroll
            for (int k = 0; k < j; ++k) {
                if (merged || ((dup >> k) & 1u)) continue;
                if (n != cplen[k] + (ctok[k] >= 0 ? 1 : 0)) continue;
                bool differ = false;
                for (int q = lane; q < n; q += 64) {
                    const int a = q < cplen[j] ? cy[j][q] : ctok[j];
                    const int c = q < cplen[k] ? cy[k][q] : ctok[k];
                    differ = differ || (a != c);
                }
                if (__ballot(differ) != 0ull) continue;
                csc[k] = rs_logaddexpf(csc[k], csc[j]);
                dup |= 1u << j;
                merged = true;
            }
        }
        // decoder rows: a hypothesis that took no token keeps its parent's; the others take the free ones, lowest first
        unsigned used = 0;
#pragma unroll
        for (int j = 0; j < MBS_MAX_K; ++j)
            if (j < n_cand && !((dup >> j) & 1u) && ctok[j] < 0) used |= 1u << ms.dec[p][cprow[j]];
        int nk = 0;
        int win = -1, win_n = 0;
        float win_norm = 0.0f, win_score = 0.0f;
        float enorm[MBS_MAX_K], esc[MBS_MAX_K];           // n-best: norm, score and length of the entries, by candidate
        int en[MBS_MAX_K];
        unsigned left = 0;                                // n-best: the entries not yet ranked
#pragma unroll
        for (int j = 0; j < MBS_MAX_K; ++j) { enorm[j] = 0.0f; esc[j] = 0.0f; en[j] = 0; }
#pragma unroll
        for (int j = 0; j < MBS_MAX_K; ++j) {
            if (j >= n_cand || ((dup >> j) & 1u)) continue;
            int d;
            if (ctok[j] < 0) d = ms.dec[p][cprow[j]];
            else { d = __ffs((int)~used) - 1; used |= 1u << d; }
            float sc = csc[j];
            if constexpr (HW) {
                if (root >= 0 && t == T - 1) sc = sc + (-hw.g.node_score[hw_node(hw.g, cctx[j], root)]);      // Finalize
                if (lane == 0) s_ctx[nk] = cctx[j];
            }
            if constexpr (LM) { if (lane == 0) s_lm[nk] = clm[j]; }
            if (lane == 0) { s_prow[nk] = cprow[j]; s_tok[nk] = ctok[j]; s_score[nk] = sc; s_dec[nk] = d; }
            const int n = cplen[j] + (ctok[j] >= 0 ? 1 : 0);
            const float norm = length_norm ? sc / (float)(n + MBS_CONTEXT) : sc;
            if (win < 0 || norm > win_norm) { win = j; win_n = n; win_norm = norm; win_score = sc; }
            if (nbest > 0 && t == T - 1) { enorm[j] = norm; esc[j] = sc; en[j] = n; left |= 1u << j; }      // (only the list reads them)
            ++nk;
        }
        if (lane == 0) { s_nnew = nk; ms.n_hyp[pn][b] = nk; }
        if (t == T - 1 && win >= 0 && nbest > 0) {        // the utterance's last frame: the ranked list (rank 0 is the winner below)
            int nh = 0;
            for (int r = 0; r < nbest; ++r) {
                int pick = -1;
                float pnorm = 0.0f;
#pragma unroll
                for (int j = 0; j < MBS_MAX_K; ++j)
                    if (((left >> j) & 1u) && (pick < 0 || enorm[j] > pnorm)) { pick = j; pnorm = enorm[j]; }
                if (pick < 0) break;                      // the last set is smaller than nbest
                left &= ~(1u << pick);
                int wprow = 0, wtok = -1, wplen = 0, n = 0;
                float wsc = 0.0f;
#pragma unroll
                for (int j = 0; j < MBS_MAX_K; ++j)
                    if (j == pick) { wprow = cprow[j]; wtok = ctok[j]; wplen = cplen[j]; n = en[j]; wsc = esc[j]; }
                if (n > out_cap) { n = out_cap; if (lane == 0) st.counters[1] = 1; }
                const size_t e = (size_t)b * nbest + r;
                const int32_t *py = ms.y[p] + (size_t)wprow * cap, *pf = ms.fr[p] + (size_t)wprow * cap;
                for (int q = lane; q < n; q += 64) {
                    ids[e * out_cap + q] = q < wplen ? py[q] : wtok;
                    frames[e * out_cap + q] = q < wplen ? pf[q] : t;
                }
                if (lane == 0) { n_ids[e] = n; scores[e] = wsc; norm_scores[e] = pnorm; }
                ++nh;
            }
            if (lane == 0) n_hyps[b] = nh;
        } else if (t == T - 1 && win >= 0) {              // the utterance's last frame: the result
            int wprow = 0, wtok = -1, wplen = 0;
#pragma unroll
            for (int j = 0; j < MBS_MAX_K; ++j) if (j == win) { wprow = cprow[j]; wtok = ctok[j]; wplen = cplen[j]; }
            int n = win_n;
            if (n > out_cap) { n = out_cap; if (lane == 0) st.counters[1] = 1; }
            const int32_t *py = ms.y[p] + (size_t)wprow * cap, *pf = ms.fr[p] + (size_t)wprow * cap;
            for (int q = lane; q < n; q += 64) {
                ids[(size_t)b * out_cap + q] = q < wplen ? py[q] : wtok;
                frames[(size_t)b * out_cap + q] = q < wplen ? pf[q] : t;
            }
            if (lane == 0) { n_ids[b] = n; scores[b] = win_score; }
        }
    }
    __syncthreads();
    if (t + 1 >= T) return;                               // nothing reads the set after the last frame

    // ---- the new set: one wave per slot copies the parent's tokens / frames (+ the token taken) and writes the record ----
    for (int k = wave; k < s_nnew; k += 4) {
        const int prow = s_prow[k], tok = s_tok[k], row = b * K + k;
        const int n = ms.len[p][prow];
        const int32_t *py = ms.y[p] + (size_t)prow * cap, *pf = ms.fr[p] + (size_t)prow * cap;
        int32_t *ny = ms.y[pn] + (size_t)row * cap, *nf = ms.fr[pn] + (size_t)row * cap;
        for (int q = lane; q < n; q += 64) { ny[q] = py[q]; nf[q] = pf[q]; }
        if (lane == 0) {
            int nn = n;
            int l0 = ms.last0[p][prow], l1 = ms.last1[p][prow];
            if (tok >= 0) {
                if (n < cap) { ny[n] = tok; nf[n] = t; nn = n + 1; }     // (n <= t < cap: at most one token per frame)
                else st.counters[1] = 1;
                l0 = l1; l1 = tok;
                const int drow = b * K + s_dec[k];
                st.token2[drow] = l0; st.token[drow] = l1;
                st.act[atomicAdd(&st.counters[0], 1)] = drow;
            }
            ms.len[pn][row] = nn; ms.score[pn][row] = s_score[k];
            ms.last0[pn][row] = l0; ms.last1[pn][row] = l1; ms.dec[pn][row] = s_dec[k];
            if constexpr (HW) ms.ctx[pn][row] = s_ctx[k];
            if constexpr (LM) ms.lmctx[pn][row] = s_lm[k];
            const int pos = atomicAdd(&st.counters[2 + pn], 1);
            st.alive[(size_t)pn * rows + pos] = row;
        }
    }
}

// the search's layout (h .. c_tmp adjacent: one memset clears the four); -> DecodeState.a_pre, writable (mbs_act_kernel fills it)
float* mbs_layout(const rs_ctx* ctx, int B, int K, int cap, bool hotwords, bool lm, rs_arena& a, DecodeState& st, MbsState& ms) {
    const rs_dims& d = ctx->d;
    const size_t rows = (size_t)B * K, state = rows * d.pred_hidden;
    st.h = a.take<float>(state); st.c = a.take<float>(state);                // (the projection kernel's state commit copies
    st.h_tmp = a.take<float>(state); st.c_tmp = a.take<float>(state);        //  h_tmp / c_tmp there; h_tmp is the decoder output)
    st.g = a.take<float>(rows * d.joint_hidden);
    float* a_pre = a.take<float>(rows * d.joint_hidden);
    st.tcur = a.take<int32_t>(rows); st.token = a.take<int32_t>(rows); st.token2 = a.take<int32_t>(rows);
    st.act = a.take<int32_t>(rows);
    for (int k = 0; k < 2; ++k) {
        ms.len[k] = a.take<int32_t>(rows); ms.score[k] = a.take<float>(rows); ms.last0[k] = a.take<int32_t>(rows);
        ms.last1[k] = a.take<int32_t>(rows); ms.dec[k] = a.take<int32_t>(rows);
    }
    st.alive = a.take<int32_t>(rows); a.take<int32_t>(rows);                 // [2][rows]: the second list follows at pitch `rows`
    for (int k = 0; k < 2; ++k) { ms.y[k] = a.take<int32_t>(rows * cap); ms.fr[k] = a.take<int32_t>(rows * cap); }
    ms.n_hyp[0] = a.take<int32_t>(B); ms.n_hyp[1] = a.take<int32_t>(B);
    st.counters = a.take<int32_t>(16);
    st.zapprox = a.take<float>(rows * (size_t)rs_joint_zstride(d));
    ms.ctx[0] = ms.ctx[1] = nullptr;
    if (hotwords) { ms.ctx[0] = a.take<int32_t>(rows); ms.ctx[1] = a.take<int32_t>(rows); }       // (after the plain layout: it is a prefix)
    ms.lmctx[0] = ms.lmctx[1] = nullptr;
    if (lm) { ms.lmctx[0] = a.take<int32_t>(rows); ms.lmctx[1] = a.take<int32_t>(rows); }         // (last: the hotword layout is a prefix)
    ms.cap = cap;
    st.a_pre = a_pre;
    st.joint_act = d.joint_act;
    return a_pre;
}

}  // namespace

size_t rs_rnnt_mbs_workspace_bytes_impl(const rs_ctx* ctx, int B, int K, int tp_max, bool hotwords, bool lm) {
    if (B <= 0 || K <= 0 || K > MBS_MAX_K || tp_max < 0) return 0;
    rs_arena a;
    DecodeState st{};
    MbsState ms;
    mbs_layout(ctx, B, K, tp_max > 0 ? tp_max : 1, hotwords || lm, lm, a, st, ms);
    return a.bytes() + RS_DECODE_SLACK;
}

int rs_rnnt_mbs_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int K, float blank_penalty,
                     int length_norm, int out_cap, int32_t* ids, int32_t* frames, int32_t* n_ids, float* scores, int nbest, float* norm_scores,
                     int32_t* n_hyps, const rs_hotwords* hotwords, const int32_t* graph_of, const rs_ngram* ngram, float lm_alpha,
                     void* workspace, size_t workspace_bytes, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const int D = d.pred_hidden, J = d.joint_hidden, V = d.n_logits;
    if (B <= 0) return RS_OK;
    if (!ctx->k2_conv_w || d.pred_layers != 1) return rs_fail(ctx, RS_EINVAL, "modified beam search: the context has no stateless decoder");
    if (int rc = rs_rnnt_check_dims(ctx, "modified beam search"); rc != RS_OK) return rc;
    if (K < 1 || K > MBS_MAX_K) return rs_fail(ctx, RS_EINVAL, "modified beam search: max_active_paths must be 1..%d", MBS_MAX_K);
    if ((long long)K * V > 0x7fffffffLL) return rs_fail(ctx, RS_EINVAL, "modified beam search: vocabulary too large");
    const int cap = tp_max > 0 ? tp_max : 1;              // at most one token per frame
    rs_arena arena(workspace);
    DecodeState st{};
    MbsState ms;
    const bool HWF = hotwords != nullptr && graph_of != nullptr && hotwords->n_graphs > 0;      // else: the plain kernels, today's bits
    const bool LMF = ngram != nullptr && ngram->n_nodes > 0 && lm_alpha != 0.0f;                // else: the forms above, today's bits
    MbsHwLm hwlm{};
    MbsHw& hw = hwlm;                                     // the hotword form takes the base: the graphs alone
    if (HWF) { hw.g = *hotwords; hw.graph_of = graph_of; }
    if (LMF) { hwlm.lm = *ngram; hwlm.alpha = lm_alpha; }
    float* const a_pre = mbs_layout(ctx, B, K, cap, HWF || LMF, LMF, arena, st, ms);
    if (workspace_bytes < arena.bytes() + RS_DECODE_SLACK)
        return rs_fail(ctx, RS_EWORKSPACE, "modified beam search: workspace %zu < %zu", workspace_bytes, arena.bytes() + RS_DECODE_SLACK);
    const int rows = B * K;
    float* const zbuf = st.zapprox;
    st.unk = rs_k2_unk_id(ctx);
    const int zstride = rs_joint_zstride(d);

    const auto init_hw = mbs_init_kernel<true>;
    const auto init = mbs_init_kernel<false>;
    // the selection kernel: the logits a lane keeps in registers follow from the vocabulary; the hotword form takes the graphs last
    auto select_hw = mbs_select_kernel<4, true>;
    if (V > MBS_THREADS * 4) select_hw = V <= MBS_THREADS * 42 ? mbs_select_kernel<42, true> : mbs_select_kernel<0, true>;
    auto select = mbs_select_kernel<4, false>;
    if (V > MBS_THREADS * 4) select = V <= MBS_THREADS * 42 ? mbs_select_kernel<42, false> : mbs_select_kernel<0, false>;
    const auto init_lm = mbs_init_kernel<true, true>;     // the LM form: the model, and the call's graphs or none
    auto select_lm = mbs_select_kernel<4, true, true>;
    if (V > MBS_THREADS * 4) select_lm = V <= MBS_THREADS * 42 ? mbs_select_kernel<42, true, true> : mbs_select_kernel<0, true, true>;
    // the search, written once: `init_k` and `select_k` are the form's kernels, `tables` their last argument (the graphs, or nothing)
    auto search = [&](auto init_k, auto select_k, const auto& tables) -> int {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
        RS_HIP(ctx, hipMemsetAsync(st.h, 0, 4 * rs_align((size_t)rows * D * 4), s));                  // h .. c_tmp are adjacent
        if (nbest > 0) {                                  // the lists: an entry that is not written has no labels, an utterance without frames no entry
            RS_HIP(ctx, hipMemsetAsync(n_ids, 0, (size_t)B * nbest * 4, s));
            RS_HIP(ctx, hipMemsetAsync(scores, 0, (size_t)B * nbest * 4, s));
            RS_HIP(ctx, hipMemsetAsync(norm_scores, 0, (size_t)B * nbest * 4, s));
            RS_HIP(ctx, hipMemsetAsync(n_hyps, 0, (size_t)B * 4, s));
        }
        hipLaunchKernelGGL(init_k, dim3(1), dim3(256), 0, s, st, ms, enc_lens, B, K, d.blank_id, nbest > 0 ? nullptr : n_ids,
                           nbest > 0 ? nullptr : scores, tables);
        if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st, rows, s); rc != RS_OK) return rc;
        RS_CHECK_LAUNCH(ctx, "modified beam search init");
        const int act_blocks = (int)(((long long)rows * (J / 4) + 255) / 256);
        for (int t = 0; t < tp_max; ++t) {
            hipLaunchKernelGGL(mbs_act_kernel, dim3(act_blocks), dim3(256), 0, s, st, ms, joint_enc, a_pre, rows, tp_max, J, K, t);
            if (int rc = rs_rnnt_launch_joint_logits_indirect(ctx, &st, joint_enc, rows, rows, tp_max, K, t, s); rc != RS_OK) return rc;
            hipLaunchKernelGGL(select_k, dim3(B), dim3(MBS_THREADS), 0, s, st, ms, zbuf, zstride, enc_lens, rows, K, V, d.blank_id, st.unk, t,
                               blank_penalty, length_norm, out_cap, ids, frames, n_ids, scores, nbest, norm_scores, n_hyps, tables);
            if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st, rows, s); rc != RS_OK) return rc;
        }
        RS_CHECK_LAUNCH(ctx, "modified beam search step");
        int32_t hc[4] = {0, 0, 0, 0};
        RS_HIP(ctx, hipMemcpyAsync(hc, st.counters, sizeof hc, hipMemcpyDeviceToHost, s));
        RS_HIP(ctx, hipStreamSynchronize(s));
        prof.end();
        if (hc[1]) return rs_fail(ctx, RS_EOVERFLOW, "modified beam search: a result has more than out_cap=%d tokens", out_cap);
        return RS_OK;
    };
    if (LMF) return search(init_lm, select_lm, hwlm);
    if (HWF) return search(init_hw, select_hw, hw);
    return search(init, select, MbsNoHw{});
}
