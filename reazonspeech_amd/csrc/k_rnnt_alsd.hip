// k_rnnt_alsd.hip — alignment-length synchronous beam search (ALSD) over the RNN-T prediction and joint networks
// (SURVEY.md §8f "next" row 2: [UPSTREAM] BeamRNNTInfer.align_length_sync_decoding, the strategy the reference's
// post-processing is written for — pkg/nemo-asr/src/decode.py:29,38-41,48).
//
// Hypotheses of all utterances advance in lockstep over the alignment index i = t + u.  Hypothesis rows are
// r = utterance * beam + slot; the prediction-network and joint kernels of the greedy path (k_rnnt.hip) run over
// those rows unchanged (exact f32, fixed accumulation order), so every number here can be compared bit for bit
// with oracle/rnnt_alsd.c, which documents the evaluation order of the search itself (log-softmax reduction tree,
// expansion / selection / recombination order, where a finished hypothesis reads its score).
//
// One alignment step = 6 launches:
//   joint logits of the live rows (rnnt_tile_kernel<2>)         -> z [rows][Vpad]
//   alsd_select_kernel (one workgroup per utterance, one wave per beam slot)
//        log-softmax + top-`beam` tokens per live hypothesis, the `beam` best expansions, recombination,
//        finished-hypothesis bookkeeping; writes the new beam's labels / alignment steps / scores (ping-pong
//        buffers), each new row's parent row, and the work lists of the next step
//   alsd_reorder_kernel   new row <- parent row's prediction-network state (h, c, g), ping-pong
//   LSTM x L + joint.pred over the rows that took a token (rnnt_lstm4 / rnnt_pred16 or the wide variants)
//
// HOTWORDS (rs_rnnt_alsd_hotwords; the graph, `step` and `Finalize` are stated in include/rs_asr.h, the walk is k_rnnt_hotwords.h,
// shared with the modified beam search).  NeMo's ALSD has no hotword rule; this one is the project's.  Every hypothesis row carries
// a node of its utterance's graph (AlsdHw.ctx, ping-pong like the records; the start hypothesis stands at the root).  Phase 1: the
// W best non-blank tokens are picked by raw logit as in the plain form; the blank candidate keeps score and state; a label
// candidate v takes (delta, s') = step(s, v), its score is (hs + (z[v] - lse)) + delta, its state s' — lane 0 of the hypothesis's
// wave walks the graph, at most W counted walks, the states live in LDS next to c_tok.  Phase 2 RANKS THE BOOSTED SCORES (the
// modified beam search adds its bonus after the selection; here a phrase continuation inside its hypothesis's top W can overtake);
// recombination is unchanged (equal label sequences have equal states; the first occurrence's stays).  A hypothesis recorded as
// finished is recorded with sc + (-node_score[state]) (Finalize), sc its score after recombination, and its normalised score is
// computed from that value; the "nothing finished" exit does the same to every beam entry before comparing.  Phase 3 writes the
// new row's state.  It is the hotword form of alsd_init_kernel / alsd_select_kernel (template parameter HW): no further launch,
// no host round trip.  The plain instantiations are the ones launched when no utterance of the call has a graph; inside the
// hotword form a workgroup whose utterance has none takes the plain statements.  Restated by tests/alsd_checker.c.
//
// N-GRAM LM (rs_rnnt_alsd_lm; the table and `step` are stated in include/rs_asr.h, the walk is k_rnnt_ngram.h).  Every hypothesis
// row carries an LM state (AlsdHwLm.lmctx, ping-pong; the start hypothesis stands at `start`).  A label candidate's score is
// ((hs + (z[v] - lse)) [+ delta]) + (alpha * lp), the product rounded first, its state the step's next state; the blank keeps score
// and state.  An LM walk usually backs off through every level (a hotword walk usually ends at the first node), so the W walks of a
// hypothesis run SIDE BY SIDE: the W picks are made as in the plain form, lane j keeps pick j in registers, and after the last pick
// lane j computes candidate j whole — score, hotword step if the utterance has a graph, LM step — and writes it to LDS (c_lm next
// to c_state).  The LM form is the template parameter LM of alsd_init_kernel / alsd_select_kernel; it is compiled with HW on and
// carries the call's graphs, or none (graph_of == nullptr: every utterance takes the no-graph statements).  Restated by
// tests/alsd_checker.c.
// Compiled with -ffp-contract=off.
#include "k_rnnt_common.h"
#include "k_rnnt_hotwords.h"
#include "k_rnnt_ngram.h"

#include <type_traits>

namespace {

constexpr int MAX_BEAM = 8;
constexpr int MAX_CAND = MAX_BEAM * (MAX_BEAM + 1);

struct AlsdState {
    // per hypothesis row; [2] = ping-pong: step i reads set (i & 1) and writes set ((i + 1) & 1)
    int32_t* len[2];     // [rows] labels emitted
    float* score[2];     // [rows]
    int32_t* y[2];       // [rows][cap] labels
    int32_t* al[2];      // [rows][cap] alignment index of each label
    int32_t* n_hyp[2];   // [B] hypotheses in the beam
    int32_t* parent;     // [rows] row whose prediction-network state the row written this step continues
    // finished hypotheses: the best one so far per utterance
    int32_t* fin_n;      // [B], -1 = none yet
    float* fin_norm;     // [B]
    float* fin_score;    // [B]
    int32_t* fin_y;      // [B][cap]
    int32_t* fin_al;     // [B][cap]
    int32_t* done;       // [B]
    int cap;
    // n-best (rs_rnnt_alsd_nbest, nbest >= 1; otherwise nbest == 0 and every pointer below is null): the ranked list of finished
    // hypotheses that stands in place of the single fin_* record.  A slot table with an order array: labels live in slots and are
    // written once per insertion, the ranks only move slot numbers.
    int nbest;
    int32_t* nb_n;       // [B] entries in the list
    int32_t* nb_slot;    // [B][MAX_BEAM] slot of rank r
    float* nb_norm;      // [B][MAX_BEAM] by rank
    float* nb_score;     // [B][MAX_BEAM] by rank
    int32_t* nb_len;     // [B][MAX_BEAM] by rank
    int32_t* nb_y;       // [B][MAX_BEAM][cap] by slot
    int32_t* nb_al;      // [B][MAX_BEAM][cap] by slot
    float* out_norm;     // [B][nbest] the caller's norm_scores
    int32_t* out_nhyps;  // [B] the caller's n_hyps
};

// ---- the ranked list in registers of wave 0 (every lane holds the same values): ranks 0 .. n - 1, best first -------------------
// RULE (include/rs_asr.h rs_rnnt_alsd_nbest): a candidate enters below every entry whose norm is >= its own (earlier-finished wins
// ties, as the single record's strict `>` does); the list holds a label sequence at most once — equal sequences can only finish in the
// same alignment step (i = T - 1 + n), so a candidate is compared with the entries that entered in THIS step only (`src`: their beam
// row, whose labels are still in as.y[p]); of two equal ones the greater norm stays, the first on a tie; a full list drops its tail.
struct AlsdList {
    int n;
    int slot[MAX_BEAM], len[MAX_BEAM], src[MAX_BEAM];
    float norm[MAX_BEAM], score[MAX_BEAM];
};

__device__ __forceinline__ void alsd_list_load(const AlsdState& as, int b, AlsdList& l) {
    l.n = as.nb_n[b];
#pragma unroll
    for (int r = 0; r < MAX_BEAM; ++r) {
        const bool in = r < l.n;
        l.slot[r] = in ? as.nb_slot[b * MAX_BEAM + r] : 0; l.len[r] = in ? as.nb_len[b * MAX_BEAM + r] : 0; l.src[r] = -1;
        l.norm[r] = in ? as.nb_norm[b * MAX_BEAM + r] : 0.0f; l.score[r] = in ? as.nb_score[b * MAX_BEAM + r] : 0.0f;
    }
}

__device__ __forceinline__ void alsd_list_store(const AlsdState& as, int b, const AlsdList& l) {      // one lane
    as.nb_n[b] = l.n;
#pragma unroll
    for (int r = 0; r < MAX_BEAM; ++r)
        if (r < l.n) {
            as.nb_slot[b * MAX_BEAM + r] = l.slot[r]; as.nb_len[b * MAX_BEAM + r] = l.len[r];
            as.nb_norm[b * MAX_BEAM + r] = l.norm[r]; as.nb_score[b * MAX_BEAM + r] = l.score[r];
        }
}

// offer beam row `row` of set p (n labels, score sc after Finalize, norm) to the list; one wave, the label copy spread over its lanes
__device__ __forceinline__ void alsd_list_offer(const AlsdState& as, int b, int p, AlsdList& l, int row, int n, float sc, float norm, int lane) {
    const int cap = as.cap;
    const int32_t* ry = as.y[p] + (size_t)row * cap;
    int dupr = -1;
#pragma unroll
    for (int r = 0; r < MAX_BEAM; ++r) {
        if (r >= l.n || dupr >= 0 || l.src[r] < 0 || l.len[r] != n) continue;      // (uniform over the wave)
        const int32_t* oy = as.y[p] + (size_t)l.src[r] * cap;
        bool differ = false;
        for (int q = lane; q < n; q += 64) differ = differ || (ry[q] != oy[q]);
        if (__ballot(differ) == 0ull) dupr = r;
    }
    int slot = -1;
    if (dupr >= 0) {                                       // the same labels finished earlier in this step
        float dn = 0.0f;
#pragma unroll
        for (int r = 0; r < MAX_BEAM; ++r) if (r == dupr) { dn = l.norm[r]; slot = l.slot[r]; }
        if (!(norm > dn)) return;                          // the first one stays on a tie
#pragma unroll
        for (int r = 0; r + 1 < MAX_BEAM; ++r)
            if (r >= dupr) { l.slot[r] = l.slot[r + 1]; l.len[r] = l.len[r + 1]; l.src[r] = l.src[r + 1]; l.norm[r] = l.norm[r + 1]; l.score[r] = l.score[r + 1]; }
        l.n -= 1;
    }
    int pos = 0;
#pragma unroll
    for (int r = 0; r < MAX_BEAM; ++r) pos += (r < l.n && l.norm[r] >= norm) ? 1 : 0;
    if (pos >= as.nbest) return;                           // a full list of better entries
    if (slot < 0) {
        if (l.n == as.nbest) {                             // the tail leaves; its slot takes the newcomer
#pragma unroll
            for (int r = 0; r < MAX_BEAM; ++r) if (r == l.n - 1) slot = l.slot[r];
            l.n -= 1;
        } else {
            slot = l.n;                                    // (slots 0 .. n - 1 are the ones in use: a slot is only ever freed to be refilled)
        }
    }
#pragma unroll
    for (int r = MAX_BEAM - 1; r >= 1; --r)
        if (r > pos && r <= l.n) { l.slot[r] = l.slot[r - 1]; l.len[r] = l.len[r - 1]; l.src[r] = l.src[r - 1]; l.norm[r] = l.norm[r - 1]; l.score[r] = l.score[r - 1]; }
#pragma unroll
    for (int r = 0; r < MAX_BEAM; ++r) if (r == pos) { l.slot[r] = slot; l.len[r] = n; l.src[r] = row; l.norm[r] = norm; l.score[r] = sc; }
    l.n += 1;
    int32_t* dy = as.nb_y + ((size_t)b * MAX_BEAM + slot) * cap;
    int32_t* dal = as.nb_al + ((size_t)b * MAX_BEAM + slot) * cap;
    const int32_t* ral = as.al[p] + (size_t)row * cap;
    for (int q = lane; q < n; q += 64) { dy[q] = ry[q]; dal[q] = ral[q]; }
}

struct AlsdNoHw {};      // the kernel argument of the plain form
struct AlsdHw {          // hotwords: the graphs of the call and the node each hypothesis row stands at
    RnntHw t;
    int32_t* ctx[2];     // [rows], ping-pong like AlsdState's records
};

struct AlsdHwLm : AlsdHw {   // n-gram LM: the model, its weight and the LM state of each hypothesis row (the graphs may be absent)
    rs_ngram g;
    float alpha;
    int32_t* lmctx[2];   // [rows], ping-pong
};
template <bool HW, bool LM>
using AlsdArg = std::conditional_t<LM, AlsdHwLm, std::conditional_t<HW, AlsdHw, AlsdNoHw>>;
// root of utterance b's graph; the LM form may carry no graphs at all
template <bool LM, class A>
__device__ __forceinline__ int alsd_root(const A& hw, int b) {
    if constexpr (LM) { if (hw.t.graph_of == nullptr) return -1; }
    return hw_root(hw.t, b);
}

// label budget of an utterance with T frames (oracle/alsd.py: a float is a multiple of T, an int is absolute)
__host__ __device__ inline int alsd_budget(int T, double ratio, int abs_len) { return abs_len >= 0 ? abs_len : (int)(ratio * (double)T); }

template <bool HW, bool LM = false>
__global__ void alsd_init_kernel(DecodeState st, AlsdState as, const int32_t* __restrict__ enc_lens, int B, int W, int blank,
                                 double ratio, int abs_len, AlsdArg<HW, LM> hw) {
    // single workgroup: the start hypothesis of every utterance and the first work lists, in row order
    __shared__ int n_alive_s;
    if (threadIdx.x == 0) n_alive_s = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int row = b * W;
        as.len[0][row] = 0; as.score[0][row] = 0.0f; as.n_hyp[0][b] = 1;
        as.fin_n[b] = -1; as.fin_norm[b] = 0.0f; as.fin_score[b] = 0.0f; as.done[b] = 0;
        if (as.nbest > 0) as.nb_n[b] = 0;
        if constexpr (HW) { const int r = alsd_root<LM>(hw, b); hw.ctx[0][row] = r < 0 ? 0 : r; }
        if constexpr (LM) hw.lmctx[0][row] = lm_node(hw.g, hw.g.start);
        st.token[row] = blank; st.tcur[row] = 0; st.act[b] = row;
        const int T = enc_lens[b];
        if (T > 0 && T + alsd_budget(T, ratio, abs_len) > 0) st.alive[atomicAdd(&n_alive_s, 1)] = row;
    }
    __syncthreads();
    // counters: [0] rows that took a token, [1] overflow flag, [2],[3] live rows of list 0 / 1, [4] finished utterances
    if (threadIdx.x == 0) { st.counters[0] = B; st.counters[1] = 0; st.counters[2] = n_alive_s; st.counters[3] = 0; st.counters[4] = 0; }
}

// label q of a candidate = its parent's label q, or the candidate's own token at the end
__device__ __forceinline__ int cand_len(int parent_len, int tok) { return parent_len + (tok >= 0 ? 1 : 0); }

// NVR > 0: the logits row of a hypothesis is read ONCE into NVR registers per lane (V <= 64 NVR), every load in flight before the
// first comparison; the scan for the maximum / the W best and the exp-sum then walk the registers in the same ascending order as
// the two memory passes of the NVR = 0 form — identical arithmetic, one memory round trip instead of two chains of 47.
// HW: the hotword form (see the head of this file); the plain form is the same text without the `if constexpr (HW)` statements.
// LM: the n-gram form (HW on as well); the other forms are the same text without the `if constexpr (LM)` statements.
// NB: the n-best form (rs_rnnt_alsd_nbest): the ranked list in place of the fin_* record.  A template parameter, not a run-time
// branch: the list's registers in the other forms cost the old entries 1.5 % (95.8 against 94.4 ms per 256 x 10 s batch).
template <int NVR, bool HW, bool LM = false, bool NB = false>
__global__ __launch_bounds__(64 * MAX_BEAM) void alsd_select_kernel(
    DecodeState st, AlsdState as, const float* __restrict__ zbuf, int zstride, const int32_t* __restrict__ enc_lens, int B, int W,
    int V, int blank, int i, double ratio, int abs_len, int score_norm, int merge, int out_cap, int32_t* __restrict__ ids,
    int32_t* __restrict__ steps, int32_t* __restrict__ n_ids, float* __restrict__ scores, AlsdArg<HW, LM> hw) {
    static_assert(HW || !LM, "the LM form is compiled with the hotword statements");
    const int b = blockIdx.x;
    if (as.done[b]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = i & 1, pn = p ^ 1;
    const int T = enc_lens[b];
    const int n_steps = T + alsd_budget(T, ratio, abs_len);
    const int n_cur = as.n_hyp[p][b];
    const int cap = as.cap;
    const int NC = W * (W + 1);

    __shared__ float c_score[MAX_CAND];
    __shared__ int c_tok[MAX_CAND];
    __shared__ int c_ok[MAX_CAND];
    __shared__ int c_state[HW ? MAX_CAND : 1];   // hotwords: the context state of each candidate
    int root = -1;                               // hotwords: the root of the utterance's graph, -1 = it has none
    if constexpr (HW) root = alsd_root<LM>(hw, b);
    __shared__ int c_lm[LM ? MAX_CAND : 1];      // n-gram LM: the LM state of each candidate
    __shared__ int s_sel[MAX_BEAM];        // selected candidate of beam position j
    __shared__ float s_score[MAX_BEAM];    // its score after recombination
    __shared__ int s_keep[MAX_BEAM];       // beam position written to new slot k
    __shared__ int s_nkeep, s_live;

    for (int c = tid; c < MAX_CAND; c += blockDim.x) c_ok[c] = 0;
    if (tid == 0) { s_live = 0; s_nkeep = 0; }
    __syncthreads();

    // ---- phase 1: one wave per hypothesis: log-softmax, blank and top-W token expansions -----------------------------
    {
        const int row = b * W + wave;
        bool live = false;
        if (i < n_steps && wave < n_cur) live = (i - as.len[p][row]) <= T - 1;
        if (live) {
            const float* zr = zbuf + (size_t)row * zstride;
            // ONE scan finds the row maximum AND each lane's own W best non-blank logits (sorted by (logit desc, index asc): a lane
            // meets its columns in ascending order, so a later equal logit never displaces an earlier one); the W best of the
            // row are then popped from the 64 sorted lists in W register rounds.  (The row used to be scanned once for the
            // maximum and once more per beam slot: 2 + W passes over 3001 logits, W of them only to find what this scan
            // already held in registers.)  The selection is the same total order as before: identical candidates.
            float m = -INFINITY;
            float tz[MAX_BEAM];
            int tv[MAX_BEAM];
#pragma unroll
            for (int k = 0; k < MAX_BEAM; ++k) { tz[k] = -INFINITY; tv[k] = -1; }
            auto scan = [&](int v, float zv) {
                if (zv > m) m = zv;
                if (v != blank) {
                    float cz = zv;
                    int cv = v;
                    bool ins = false;                                       // once placed, everything behind shifts down one slot
#pragma unroll
                    for (int k = 0; k < MAX_BEAM; ++k) {
                        if (k < W && (ins || tv[k] < 0 || cz > tz[k])) {   // an empty slot takes anything (also a -inf logit)
                            const float sz = tz[k]; const int sv = tv[k];
                            tz[k] = cz; tv[k] = cv;
                            cz = sz; cv = sv;
                            ins = true;
                        }
                    }
                }
            };
            float zreg[NVR > 0 ? NVR : 1];
            if constexpr (NVR > 0) {
#pragma unroll
                for (int q = 0; q < NVR; ++q) {
                    const int v = lane + 64 * q;
                    zreg[q] = zr[v < V ? v : V - 1];
                }
#pragma unroll
                for (int q = 0; q < NVR; ++q) {
                    const int v = lane + 64 * q;
                    if (v < V) scan(v, zreg[q]);
                }
            } else {
                for (int v = lane; v < V; v += 64) scan(v, zr[v]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(m, off, 64); if (o > m) m = o; }
            float sum = 0.0f;
            if constexpr (NVR > 0) {
#pragma unroll
                for (int q = 0; q < NVR; ++q)
                    if (lane + 64 * q < V) sum = sum + rs_expf(zreg[q] - m);
            } else {
                for (int v = lane; v < V; v += 64) sum = sum + rs_expf(zr[v] - m);
            }
            sum = wave_sum(sum);
            sum = __shfl(sum, 0, 64);
            const float lse = m + rs_logf(sum);
            const float hs = as.score[p][row];
            const int base = wave * (W + 1);
            if (lane == 0) { c_score[base] = hs + (zr[blank] - lse); c_tok[base] = -1; c_ok[base] = 1; s_live = 1; }
            int hstate = 0;                                                  // hotwords: the node this hypothesis stands at
            if constexpr (HW) {
                if (root >= 0) hstate = hw.ctx[p][row];
                if (lane == 0) c_state[base] = hstate;                       // the blank keeps it
            }
            [[maybe_unused]] int lstate = 0, n_pick = 0, mv = -1;            // n-gram LM: the row's state; lane j keeps pick j
            [[maybe_unused]] float mz = 0.0f;
            if constexpr (LM) {
                lstate = hw.lmctx[p][row];
                if (lane == 0) c_lm[base] = lstate;                          // the blank keeps it
            }
            for (int j = 0; j < W; ++j) {
                float bz = tz[0];
                int bv = tv[0];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const float oz = __shfl_xor(bz, off, 64);
                    const int ov = __shfl_xor(bv, off, 64);
                    if (ov >= 0 && (bv < 0 || oz > bz || (oz == bz && ov < bv))) { bz = oz; bv = ov; }
                }
                if (bv < 0) break;
                if constexpr (LM) {
                    if (lane == j) { mz = bz; mv = bv; }
                    n_pick = j + 1;
                } else if (lane == 0) {
                    float cs = hs + (bz - lse);
                    if constexpr (HW) {
                        int nx = 0;
                        if (root >= 0) { const float delta = hw_step(hw.t.g, root, hstate, bv, &nx); cs = cs + delta; }
                        c_state[base + 1 + j] = nx;
                    }
                    c_score[base + 1 + j] = cs; c_tok[base + 1 + j] = bv; c_ok[base + 1 + j] = 1;
                }
                if (tv[0] == bv) {                                           // the owner pops its head
#pragma unroll
                    for (int k = 0; k + 1 < MAX_BEAM; ++k) { tz[k] = tz[k + 1]; tv[k] = tv[k + 1]; }
                    tz[MAX_BEAM - 1] = -INFINITY; tv[MAX_BEAM - 1] = -1;
                }
            }
            if constexpr (LM) {
                if (lane < n_pick) {                                         // candidate `lane`, whole: W walks side by side
                    float cs = hs + (mz - lse);
                    int nx = 0, ln = 0;
                    if (root >= 0) { const float delta = hw_step(hw.t.g, root, hstate, mv, &nx); cs = cs + delta; }
                    const float lp = lm_step(hw.g, lstate, mv, &ln);
                    cs = cs + (hw.alpha * lp);
                    c_state[base + 1 + lane] = nx; c_lm[base + 1 + lane] = ln;
                    c_score[base + 1 + lane] = cs; c_tok[base + 1 + lane] = mv; c_ok[base + 1 + lane] = 1;
                }
            }
        }
    }
    __syncthreads();

    if (!s_live) {
        // ---- the search of this utterance is over (alignment budget spent, or every hypothesis is past the last frame)
        if constexpr (NB) {
          if (wave == 0) {
            // the ranked list; nothing finished: the beam's entries under the same ranking and de-duplication
            AlsdList l;
            alsd_list_load(as, b, l);
            if (l.n == 0) {
                for (int s = 0; s < n_cur; ++s) {
                    const int row = b * W + s;
                    const int n = as.len[p][row];
                    float sc = as.score[p][row];
                    if constexpr (HW) {
                        if (root >= 0) sc = sc + (-hw.t.g.node_score[hw_node(hw.t.g, hw.ctx[p][row], root)]);      // Finalize
                    }
                    const float norm = score_norm ? sc / (float)(n + 1) : sc;
                    alsd_list_offer(as, b, p, l, row, n, sc, norm, lane);
                }
            }
            const int nbest = as.nbest;
            for (int r = 0; r < nbest; ++r) {
                const size_t e = (size_t)b * nbest + r;
                if (r >= l.n) { if (lane == 0) n_ids[e] = 0; continue; }
                int slot = 0, n = 0;
                float sc = 0.0f, norm = 0.0f;
#pragma unroll
                for (int k = 0; k < MAX_BEAM; ++k) if (k == r) { slot = l.slot[k]; n = l.len[k]; sc = l.score[k]; norm = l.norm[k]; }
                if (n > out_cap) { n = out_cap; if (lane == 0) st.counters[1] = 1; }
                const int32_t* sy = as.nb_y + ((size_t)b * MAX_BEAM + slot) * cap;       // (a lane reads back the positions it wrote)
                const int32_t* sal = as.nb_al + ((size_t)b * MAX_BEAM + slot) * cap;
                for (int q = lane; q < n; q += 64) { ids[e * out_cap + q] = sy[q]; steps[e * out_cap + q] = sal[q]; }
                if (lane == 0) { n_ids[e] = n; scores[e] = sc; as.out_norm[e] = norm; }
            }
            if (lane == 0) { as.out_nhyps[b] = l.n; as.done[b] = 1; atomicAdd(&st.counters[4], 1); }
          }
          return;
        }
        if (wave == 0) {
            int src_n = as.fin_n[b];
            float src_score = as.fin_score[b];
            const int32_t *src_y = as.fin_y + (size_t)b * cap, *src_al = as.fin_al + (size_t)b * cap;
            if (src_n < 0) {   // nothing finished: the best of the beam
                float bn = 0.0f;
                for (int s = 0; s < n_cur; ++s) {
                    const int row = b * W + s;
                    const int n = as.len[p][row];
                    float sc = as.score[p][row];
                    if constexpr (HW) {
                        if (root >= 0) sc = sc + (-hw.t.g.node_score[hw_node(hw.t.g, hw.ctx[p][row], root)]);      // Finalize
                    }
                    const float norm = score_norm ? sc / (float)(n + 1) : sc;
                    if (src_n < 0 || norm > bn) {
                        src_n = n; src_score = sc; bn = norm;
                        src_y = as.y[p] + (size_t)row * cap; src_al = as.al[p] + (size_t)row * cap;
                    }
                }
            }
            int n = src_n < 0 ? 0 : src_n;
            if (n > out_cap) { n = out_cap; if (lane == 0) st.counters[1] = 1; }
            for (int q = lane; q < n; q += 64) { ids[(size_t)b * out_cap + q] = src_y[q]; steps[(size_t)b * out_cap + q] = src_al[q]; }
            if (lane == 0) { n_ids[b] = n; scores[b] = src_score; as.done[b] = 1; atomicAdd(&st.counters[4], 1); }
        }
        return;
    }

    // ---- phase 2 (wave 0, every lane computes the same values): selection, recombination, finished hypotheses ---------
    if (wave == 0) {
        for (int c = lane; c < NC; c += 64) {
            if (!c_ok[c]) continue;
            const float sc = c_score[c];
            int rank = 0;
            for (int o = 0; o < NC; ++o)
                if (c_ok[o] && (c_score[o] > sc || (c_score[o] == sc && o < c))) ++rank;
            if (rank < W) s_sel[rank] = c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        int n_valid = 0;
        for (int c = lane; c < NC; c += 64) n_valid += c_ok[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n_valid += __shfl_xor(n_valid, off, 64);
        const int n_sel = n_valid < W ? n_valid : W;
        int sel[MAX_BEAM], stok[MAX_BEAM], splen[MAX_BEAM];
        float ssc[MAX_BEAM];
        const int32_t* sy[MAX_BEAM];
        unsigned dup = 0;
#pragma unroll
        for (int j = 0; j < MAX_BEAM; ++j) {
            sel[j] = 0; stok[j] = -1; splen[j] = 0; ssc[j] = 0.0f; sy[j] = as.y[p];
            if (j < n_sel) {
                sel[j] = s_sel[j];
                ssc[j] = c_score[sel[j]];
                stok[j] = c_tok[sel[j]];
                const int prow = b * W + sel[j] / (W + 1);
                splen[j] = as.len[p][prow];
                sy[j] = as.y[p] + (size_t)prow * cap;
            }
        }
        // recombination: equal label sequences add into the first occurrence
#pragma unroll
        for (int j = 1; j < MAX_BEAM; ++j) {
            if (j >= n_sel) continue;
            bool merged = false;
#pragma unroll
            for (int k = 0; k < j; ++k) {
                if (merged || ((dup >> k) & 1u)) continue;
                const int n = cand_len(splen[j], stok[j]);
                if (n != cand_len(splen[k], stok[k])) continue;
                bool differ = false;
                for (int q = lane; q < n; q += 64) {
                    const int a = q < splen[j] ? sy[j][q] : stok[j];
                    const int c = q < splen[k] ? sy[k][q] : stok[k];
                    differ = differ || (a != c);
                }
                if (__ballot(differ) != 0ull) continue;
                ssc[k] = rs_logaddexpf(ssc[k], ssc[j]);
                dup |= 1u << j;
                merged = true;
            }
        }
        // finished hypotheses: a blank taken at the last frame; the score is read after recombination
        [[maybe_unused]] AlsdList nl;
        if constexpr (NB) alsd_list_load(as, b, nl);
        int fn = as.fin_n[b];
        float fnorm = as.fin_norm[b], fscore = as.fin_score[b];
        for (int s = 0; s < n_cur; ++s) {
            const int c = s * (W + 1);
            if (!c_ok[c]) continue;
            const int row = b * W + s;
            const int n = as.len[p][row];
            if (i - n != T - 1) continue;
            float sc = c_score[c];
#pragma unroll
            for (int j = 0; j < MAX_BEAM; ++j) if (j < n_sel && sel[j] == c) sc = ssc[j];
            if constexpr (HW) {
                if (root >= 0) sc = sc + (-hw.t.g.node_score[hw_node(hw.t.g, c_state[c], root)]);                  // Finalize
            }
            const float norm = score_norm ? sc / (float)(n + 1) : sc;
            if constexpr (NB) { alsd_list_offer(as, b, p, nl, row, n, sc, norm, lane); continue; }      // the list in place of the record
            if (fn < 0 || norm > fnorm) {
                fn = n; fnorm = norm; fscore = sc;
                for (int q = lane; q < n; q += 64) {
                    as.fin_y[(size_t)b * cap + q] = as.y[p][(size_t)row * cap + q];
                    as.fin_al[(size_t)b * cap + q] = as.al[p][(size_t)row * cap + q];
                }
            }
        }
        if (lane == 0) { as.fin_n[b] = fn; as.fin_norm[b] = fnorm; as.fin_score[b] = fscore; }
        if constexpr (NB) { if (lane == 0) alsd_list_store(as, b, nl); }
        // the new beam, in selection order ("merge" drops the duplicates)
        int nk = 0;
#pragma unroll
        for (int j = 0; j < MAX_BEAM; ++j) {
            if (j >= n_sel || (merge && ((dup >> j) & 1u))) continue;
            if (lane == 0) { s_keep[nk] = sel[j]; s_score[nk] = ssc[j]; }
            ++nk;
        }
        if (lane == 0) { s_nkeep = nk; as.n_hyp[pn][b] = nk; }
    }
    __syncthreads();

    // ---- phase 3: one wave per new beam slot: labels and alignment steps of the parent (+ the token taken) -------------
    if (wave < s_nkeep) {
        const int c = s_keep[wave];
        const int tok = c_tok[c];
        const int prow = b * W + c / (W + 1), row = b * W + wave;
        const int n = as.len[p][prow];
        const int32_t *py = as.y[p] + (size_t)prow * cap, *pal = as.al[p] + (size_t)prow * cap;
        int32_t *ny = as.y[pn] + (size_t)row * cap, *nal = as.al[pn] + (size_t)row * cap;
        for (int q = lane; q < n; q += 64) { ny[q] = py[q]; nal[q] = pal[q]; }
        if (lane == 0) {
            int nn = n;
            if (tok >= 0) {
                if (n < cap) { ny[n] = tok; nal[n] = i; nn = n + 1; }
                else st.counters[1] = 1;
                st.token[row] = tok;
                st.act[atomicAdd(&st.counters[0], 1)] = row;
            }
            as.len[pn][row] = nn;
            as.score[pn][row] = s_score[wave];
            as.parent[row] = prow;
            if constexpr (HW) hw.ctx[pn][row] = root >= 0 ? c_state[c] : 0;
            if constexpr (LM) hw.lmctx[pn][row] = c_lm[c];
            const int tn = (i + 1) - nn;
            st.tcur[row] = tn;
            if (i + 1 < n_steps && tn <= T - 1) {
                const int pos = atomicAdd(&st.counters[2 + ((i + 1) & 1)], 1);
                st.alive[(size_t)((i + 1) & 1) * (B * W) + pos] = row;
            }
        }
    }
}

// new row <- parent row's prediction-network state; src/dst are the two state sets
__global__ __launch_bounds__(256) void alsd_reorder_kernel(AlsdState as, int pn, int W, int rows, int L, int H, int J,
                                                           const float* __restrict__ h_src, const float* __restrict__ c_src,
                                                           const float* __restrict__ g_src, float* __restrict__ h_dst,
                                                           float* __restrict__ c_dst, float* __restrict__ g_dst) {
    const int row = blockIdx.x, b = row / W, slot = row % W;
    if (as.done[b] || slot >= as.n_hyp[pn][b]) return;
    const int prow = as.parent[row];
    for (int l = 0; l < L; ++l) {
        const size_t so = ((size_t)l * rows + prow) * H, dof = ((size_t)l * rows + row) * H;
        for (int k = 4 * threadIdx.x; k < H; k += 4 * blockDim.x) {
            *reinterpret_cast<float4*>(h_dst + dof + k) = *reinterpret_cast<const float4*>(h_src + so + k);
            *reinterpret_cast<float4*>(c_dst + dof + k) = *reinterpret_cast<const float4*>(c_src + so + k);
        }
    }
    for (int k = 4 * threadIdx.x; k < J; k += 4 * blockDim.x)
        *reinterpret_cast<float4*>(g_dst + (size_t)row * J + k) = *reinterpret_cast<const float4*>(g_src + (size_t)prow * J + k);
}

// the search's layout: two ping-pong sets of the prediction-network state (st[k].h / .c / .g; everything else of st[0] and st[1] is
// shared) and the hypothesis store
void alsd_layout(const rs_ctx* ctx, int B, int W, int cap, bool hotwords, bool lm, int nbest, rs_arena& a, DecodeState st[2], AlsdState& as,
                 int32_t* hw_ctx[2], int32_t* lm_ctx[2]) {
    const rs_dims& d = ctx->d;
    const size_t rows = (size_t)B * W, state = (size_t)d.pred_layers * rows * d.pred_hidden, J = d.joint_hidden;
    DecodeState q{};
    q.joint_act = d.joint_act;
    q.h = a.take<float>(state); q.c = a.take<float>(state);                  // adjacent: one memset
    float* h1 = a.take<float>(state); float* c1 = a.take<float>(state);
    q.h_tmp = a.take<float>(state); q.c_tmp = a.take<float>(state);
    q.g = a.take<float>(rows * J); float* g1 = a.take<float>(rows * J);
    q.tcur = a.take<int32_t>(rows); q.sym = a.take<int32_t>(rows);
    q.token = a.take<int32_t>(rows); q.act = a.take<int32_t>(rows);
    as.parent = a.take<int32_t>(rows);
    as.len[0] = a.take<int32_t>(rows); as.len[1] = a.take<int32_t>(rows);
    as.score[0] = a.take<float>(rows); as.score[1] = a.take<float>(rows);
    q.alive = a.take<int32_t>(rows); a.take<int32_t>(rows);                  // [2][rows]: the second list follows at pitch `rows`
    as.y[0] = a.take<int32_t>(rows * cap); as.y[1] = a.take<int32_t>(rows * cap);
    as.al[0] = a.take<int32_t>(rows * cap); as.al[1] = a.take<int32_t>(rows * cap);
    as.n_hyp[0] = a.take<int32_t>(B); as.n_hyp[1] = a.take<int32_t>(B);
    as.fin_n = a.take<int32_t>(B); as.fin_norm = a.take<float>(B); as.fin_score = a.take<float>(B);
    as.done = a.take<int32_t>(B);
    as.fin_y = a.take<int32_t>((size_t)B * cap); as.fin_al = a.take<int32_t>((size_t)B * cap);
    q.counters = a.take<int32_t>(16);
    q.zapprox = a.take<float>(rows * (size_t)rs_joint_zstride(d));
    hw_ctx[0] = hw_ctx[1] = nullptr;
    if (hotwords) { hw_ctx[0] = a.take<int32_t>(rows); hw_ctx[1] = a.take<int32_t>(rows); }       // (last: the plain layout is a prefix)
    lm_ctx[0] = lm_ctx[1] = nullptr;
    if (lm) { lm_ctx[0] = a.take<int32_t>(rows); lm_ctx[1] = a.take<int32_t>(rows); }             // (after them: the hotword layout is a prefix)
    as.nbest = nbest;                                                                             // (last of all: every other layout is a prefix)
    as.nb_n = as.nb_slot = as.nb_len = as.nb_y = as.nb_al = as.out_nhyps = nullptr;
    as.nb_norm = as.nb_score = as.out_norm = nullptr;
    if (nbest > 0) {
        const size_t e = (size_t)B * MAX_BEAM;
        as.nb_n = a.take<int32_t>(B); as.nb_slot = a.take<int32_t>(e); as.nb_len = a.take<int32_t>(e);
        as.nb_norm = a.take<float>(e); as.nb_score = a.take<float>(e);
        as.nb_y = a.take<int32_t>(e * cap); as.nb_al = a.take<int32_t>(e * cap);
    }
    as.cap = cap;
    st[0] = st[1] = q;
    st[1].h = h1; st[1].c = c1; st[1].g = g1;
}

}  // namespace

size_t rs_rnnt_alsd_workspace_bytes_impl(const rs_ctx* ctx, int B, int beam, int cap, bool hotwords, bool lm, int nbest) {
    if (B <= 0 || beam <= 0 || cap <= 0) return 0;
    rs_arena a;
    DecodeState st[2];
    AlsdState as;
    int32_t *hw_ctx[2], *lm_ctx[2];
    alsd_layout(ctx, B, beam, cap, hotwords || lm, lm, nbest, a, st, as, hw_ctx, lm_ctx);
    return a.bytes() + RS_DECODE_SLACK;
}

int rs_rnnt_alsd_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, int beam, double ratio,
                      int abs_len, int score_norm, int merge, int out_cap, int32_t* ids, int32_t* steps, int32_t* n_ids,
                      float* scores, int nbest, float* norm_scores, int32_t* n_hyps, const rs_hotwords* hotwords, const int32_t* graph_of,
                      const rs_ngram* ngram, float lm_alpha, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const int L = d.pred_layers, H = d.pred_hidden, J = d.joint_hidden, V = d.n_logits;
    if (B <= 0) return RS_OK;
    if (int rc = rs_rnnt_check_dims(ctx, "alsd"); rc != RS_OK) return rc;
    const int W = beam < V - 1 ? beam : V - 1;
    if (W < 1 || W > MAX_BEAM) return rs_fail(ctx, RS_EINVAL, "alsd: beam size must be 1..%d", MAX_BEAM);
    const int max_steps = tp_max + alsd_budget(tp_max, ratio, abs_len);      // >= every utterance's alignment length
    const int cap = max_steps > 0 ? max_steps : 1;
    rs_arena arena(workspace);
    DecodeState st[2];
    AlsdState as;
    const bool HWF = hotwords != nullptr && graph_of != nullptr && hotwords->n_graphs > 0;      // else: the plain kernels, today's bits
    const bool LMF = ngram != nullptr && ngram->n_nodes > 0 && lm_alpha != 0.0f;                // else: the forms above, today's bits
    AlsdHwLm hw{};
    if (HWF) { hw.t.g = *hotwords; hw.t.graph_of = graph_of; }
    if (LMF) { hw.g = *ngram; hw.alpha = lm_alpha; }
    alsd_layout(ctx, B, W, cap, HWF || LMF, LMF, nbest, arena, st, as, hw.ctx, hw.lmctx);
    as.out_norm = norm_scores; as.out_nhyps = n_hyps;
    const AlsdHw& hw_only = hw;                                                                 // the hotword form's argument
    if (workspace_bytes < arena.bytes() + RS_DECODE_SLACK)
        return rs_fail(ctx, RS_EWORKSPACE, "alsd: workspace %zu < %zu", workspace_bytes, arena.bytes() + RS_DECODE_SLACK);
    const int rows = B * W;
    float* const hset[2] = {st[0].h, st[1].h}; float* const cset[2] = {st[0].c, st[1].c}; float* const gset[2] = {st[0].g, st[1].g};
    int32_t* const counters = st[0].counters;
    float* const zbuf = st[0].zapprox;
    const int zstride = rs_joint_zstride(d);
    const auto select = V <= 64 * 48 ? alsd_select_kernel<48, false> : alsd_select_kernel<0, false>;   // (48: the logits row fits a lane's registers)
    const auto select_hw = V <= 64 * 48 ? alsd_select_kernel<48, true> : alsd_select_kernel<0, true>;  // the hotword form takes the graphs last
    const auto select_lm = V <= 64 * 48 ? alsd_select_kernel<48, true, true> : alsd_select_kernel<0, true, true>;   // the LM form: graphs and model
    // the n-best forms of the three (rs_rnnt_alsd_nbest)
    const auto select_nb = V <= 64 * 48 ? alsd_select_kernel<48, false, false, true> : alsd_select_kernel<0, false, false, true>;
    const auto select_hw_nb = V <= 64 * 48 ? alsd_select_kernel<48, true, false, true> : alsd_select_kernel<0, true, false, true>;
    const auto select_lm_nb = V <= 64 * 48 ? alsd_select_kernel<48, true, true, true> : alsd_select_kernel<0, true, true, true>;
    const auto init_lm = alsd_init_kernel<true, true>;
    const auto init_hw = alsd_init_kernel<true>;
    const auto init = alsd_init_kernel<false>;

    // the search, written once: `init_k` and `select_k` are the form's kernels, `tables` their last argument (graphs, model, or nothing)
    auto search = [&](auto init_k, auto select_k, const auto& tables) -> int {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
        RS_HIP(ctx, hipMemsetAsync(hset[0], 0, 2 * rs_align((size_t)L * rows * H * 4), s));   // h and c of set 0
        hipLaunchKernelGGL(init_k, dim3(1), dim3(256), 0, s, st[0], as, enc_lens, B, W, d.blank_id, ratio, abs_len, tables);
        // start of sequence: blank token from zero state, slot 0 of every utterance (list built by the init kernel)
        if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st[0], rows, s); rc != RS_OK) return rc;
        RS_CHECK_LAUNCH(ctx, "alsd init");

        const int CHUNK = 16;
        int32_t hc[8] = {0};
        bool finished = false;
        int i = 0;
        while (!finished && i <= max_steps) {
            for (int c = 0; c < CHUNK && i <= max_steps; ++c, ++i) {
                const int p = i & 1, pn = p ^ 1;
                if (int rc = rs_rnnt_launch_joint_logits(ctx, &st[p], joint_enc, rows, tp_max, W, i, s); rc != RS_OK) return rc;
                hipLaunchKernelGGL(select_k, dim3(B), dim3(64 * W), 0, s, st[p], as, zbuf, zstride, enc_lens, B, W, V, d.blank_id, i, ratio, abs_len,
                                   score_norm, merge, out_cap, ids, steps, n_ids, scores, tables);
                hipLaunchKernelGGL(alsd_reorder_kernel, dim3(rows), dim3(256), 0, s, as, pn, W, rows, L, H, J, hset[p], cset[p],
                                   gset[p], hset[pn], cset[pn], gset[pn]);
                if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st[pn], rows, s); rc != RS_OK) return rc;
            }
            RS_CHECK_LAUNCH(ctx, "alsd step");
            RS_HIP(ctx, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, s));
            RS_HIP(ctx, hipStreamSynchronize(s));
            finished = hc[4] >= B;
        }
        prof.end();
        if (!finished) return rs_fail(ctx, RS_ESTATE, "alsd: %d of %d utterances unfinished after %d alignment steps", B - hc[4], B, max_steps + 1);
        if (hc[1]) return rs_fail(ctx, RS_EOVERFLOW, "alsd: a hypothesis has more than out_cap=%d labels", out_cap);
        return RS_OK;
    };
    if (nbest > 0) {
        if (LMF) return search(init_lm, select_lm_nb, hw);
        if (HWF) return search(init_hw, select_hw_nb, hw_only);
        return search(init, select_nb, AlsdNoHw{});
    }
    if (LMF) return search(init_lm, select_lm, hw);
    if (HWF) return search(init_hw, select_hw, hw_only);
    return search(init, select, AlsdNoHw{});
}
