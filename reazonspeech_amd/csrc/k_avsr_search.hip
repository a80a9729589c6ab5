// k_avsr_search.hip — the two searches of AVHubertForConditionalGeneration.generate() on the device: what transformers'
// GenerationMixin._sample (do_sample False) and ._beam_search (v4.50+, early_stopping False, one eos token) do with the logits of
// every step (pkg/avsr/src/avhubert/modeling_avhubert.py:216,372-391; pkg/avsr/README.rst:41 `generate(**inputs, num_beams=5,
// max_new_tokens=256)`).  The same algorithm as reazonspeech_amd/avsr/generation.py (the host path) and oracle/avsr.py:158-227;
// restated for the CPU, operation for operation, in tests/avsr_search_checker.c.
//
// One launch per step and search (no kernel waits on another workgroup; the host loop is bounded by max_new_tokens):
//
//   avsr_greedy_step_kernel   one workgroup per row: argmax over v < V (equal values: the lower index), pad for rows that already
//                             emitted eos, the row's next decoder token, and the count of rows still unfinished
//   avsr_beam_step_kernel     one workgroup of 256 threads per clip, K <= 8 hypothesis rows:
//       1. log-softmax        per row k: m = max_v x[v]; S = sum_v rs_expf(x[v] - m); logp[v] = ((x[v] - m) - rs_logf(S)) + run_score[k]
//       2. top 2 K            of the K V values logp[k][v], by value descending, then flat index k V + v ascending: 2 K rounds, each
//                             the minimum in that order among the values after the previous pick (the rows are re-read from
//                             global memory / L2 every round: nothing of size K V is held in LDS or registers)
//       3. bookkeeping        thread 0 restates generation.py's float32 lines on the 2 K candidates (below); then all threads copy
//                             the token prefixes from the step's source buffers to its destination buffers
//
// SUMMATION ORDER of S (the only rounding-order choice in this file; max and the selection are exact in any order):
//   thread t of 256 owns the columns v = t, t + 256, t + 512, ... and adds their rs_expf terms to a zero in increasing v;
//   the 256 partial sums are then combined by a binary tree in LDS: for stride = 128, 64, ..., 1: p[t] += p[t + stride] for t < stride;
//   S = p[0].  rs_expf / rs_logf are k_rnnt_common.h's (oracle/rnnt_math.h on the host); the file is compiled with -ffp-contract=off.
//
// BOOKKEEPING, with cur = step + 1 (the position being written), den = (float)pow((double)cur, (double)length_penalty) computed on
// the host, NEG = -1e9f, candidates j = 0 .. 2K-1 in the order of (2.), parent = idx / V, token = idx % V:
//   ends[j]   = token == eos || cur + 1 >= max_len
//   lp_run[j] = top_lp[j] + (ends[j] ? 1.0f : 0.0f) * NEG;  the K largest, equal values in candidate order, run on
//   just[j]   = ends[j] && j < K                            (only one of the K best may finish)
//   lp_fin[j] = ((top_lp[j] / den) + (can_improve ? 0.0f : 1.0f) * NEG) + (just[j] ? 0.0f : 1.0f) * NEG
//   the K largest of [fin_score[0..K), lp_fin[0..2K)], equal values keeping the earlier position, are the new finished slots
//   can_improve &= any_j (run_score'[0] / den > (is_fin'[j] ? min_i fin_score'[i] : NEG))
//   the clip adds (can_improve ? 1 : 0) + (all_j ends[j] ? 0 : 0x10000) to the step's word go[step + 1]
// The search goes on after a step iff some clip can improve and some clip has a candidate that does not end: both halves of the
// word non-zero.  A step whose go[step] word says stop returns at once and leaves go[step + 1] zero, so every later step does too.
// A clip that cannot improve any more keeps extending its running beams until the global stop, as transformers does.
//
// OPTIONS (rs_avsr_search_opts; transformers' logits processors and beam-search switches).  Neutral options take the code path
// above unchanged (the <false> instantiations).  Otherwise, per step and hypothesis row, one byte per token in LDS (K Vp bytes up to
// MARK_LDS_BYTES, else in the search state) is built from the row's own prefix run_seq[step & 1][0 .. step], bos included:
//   0 untouched, 1 seen (repetition penalty), 2 banned (the token would complete an n-gram of the prefix, or it is eos while fewer
//   than min_new_tokens tokens exist).  Every banned n-gram token is also a seen one, so 2 overwrites 1 after a barrier; bytes are
//   written with plain stores of one value, so no atomics are needed.
// The processed score of (row, v) is then an O(1) lookup wherever a score is read, in transformers' order (_get_logits_processor):
//   s = seen ? (s < 0 ? s * penalty : s / penalty) : s;  s = banned ? -inf : s
// greedy: s is the raw logit, before the argmax.  beam: s = (x[v] - m) - rs_logf(S), i.e. after the log-softmax and before the
// running score is added; m and S stay those of the raw logits (no renormalisation).  -inf candidates keep the total order (value
// descending, flat index ascending).
//   early_stopping 1 (True): lp_fin[j] gets one more term first, (top_lp[j] / den) + (all K slots were finished before ? 1 : 0) * NEG;
//       the clip adds 1 to a second word go2[step + 1] unless all its K slots are finished now, and a zero go2 word stops the search
//   early_stopping 2 ("never") with length_penalty > 0: can_improve divides by den_heur = (float)pow(max_new_tokens, length_penalty)
//       instead of den (host-computed; den_heur == den otherwise)
//   num_return_sequences n: the finish kernel writes the n best finished slots of every clip, clip-major
//
// RECORDING (the _scored entry points; the <.., true> instantiations; transformers' output_scores / beam_indices /
// compute_transition_scores).  Nothing the search decides changes.  Beside run_seq / fin_seq every hypothesis row keeps, per sequence
// position pos = p + 1 of generated position p, in buffers with the same ping-pong, re-parented and copied into the finished slots in
// the same places:
//   tok_score   the processed score s of the token chosen there, transformers' scores[p][row][token]: greedy, the logit after the
//               processors; beam, (x[v] - m) - rs_logf(S) after the processors and before the running score is added
//   tok_lse     the log-sum-exp of that row's processed scores s[v], v < V, at that step (normalize_logits=True subtracts it)
//   beam_idx    beam only: the flat row clip * beams + beam the token was taken from (that step's src_rows; transformers' beam_indices)
// SUMMATION ORDER of Z (tok_lse), the same as S's: M = max_v s[v] (exact in any order); thread t of 256 owns the columns v = t, t + 256,
//   ... and adds rs_expf(s[v] - M) to a zero in increasing v, where a banned (-inf) column adds exactly 0.0f and is not passed through
//   rs_expf; the 256 partial sums are combined by the binary tree of stride 128, 64, ..., 1; lse = M + rs_logf(Z).  A row whose every
//   column is -inf has lse = -inf.  This is one more max pass and one more sum pass over the clip's K rows, re-read from global
//   memory / L2 like the selection rounds; nothing of size K V goes into LDS.
// With a dump pointer the max pass also stores the whole processed row: step_scores[step][row][v] = s[v] for v < V (-inf where
// banned) and 0 for V <= v < Vp, rows in the order the step read them (transformers' `scores` tuple); only steps that ran write.
// The finish kernel writes token_scores / token_lse / beam_indices [B n][max_new_tokens] for the n returned hypotheses of every clip;
// positions past a hypothesis' generated tokens (eos included), and slots that never finished, hold 0.0f / 0.0f / -1.
// Restated for the CPU, operation for operation, in tests/avsr_token_scores_checker.c.
//
// State buffers ping-pong by step parity: step s reads run_seq / fin_seq [s & 1] and writes [(s + 1) & 1]; positions beyond the
// ones a step writes still hold pad_token_id from rs_avsr_search_begin.
#include <math.h>

#include "k_rnnt_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXK = 8;
constexpr int LAG = 2;          // rs_avsr_generate: the host runs at most this many steps ahead of the stop word it has read
constexpr int MARK_LDS_BYTES = 32768;   // the token marks of a clip's K rows live in LDS up to this size, else in the search state

// the options as the kernels see them
struct OptArgs {
    float penalty;
    int ngram, min_new, es_true;
    int32_t* go2;               // early_stopping True: clips with an unfinished slot, per step (null otherwise)
    uint8_t* marks;             // [rows][Vp] in the search state, or null: LDS
};

struct SearchPtrs {
    int32_t *tok, *src, *run_seq, *fin_seq, *fin_len, *is_fin, *can, *last, *go;
    float *run_score, *fin_score;
    int32_t* go2;
    uint8_t* marks;
    // recording (null otherwise): [2][rows][max_len] like run_seq / fin_seq, indexed by sequence position (position 0 unused)
    float *run_ts, *run_tl, *fin_ts, *fin_tl;
    int32_t *run_bi, *fin_bi;
};
constexpr size_t SEARCH_SLACK = 256;
// the search state's layout.  go2_words / rec / mark_bytes: the pieces the options and the recording add behind the plain layout (0: not
// taken, the pointer is null); the marks come last: they are the one piece whose size depends on the vocabulary
SearchPtrs search_layout(int B, int K, int max_len, size_t go2_words, size_t mark_bytes, bool rec, rs_arena& a) {
    SearchPtrs p;
    const size_t R = (size_t)B * K;
    p.tok = a.take<int32_t>(R); p.src = a.take<int32_t>(R);
    p.run_seq = a.take<int32_t>(2 * R * max_len); p.fin_seq = a.take<int32_t>(2 * R * max_len);
    p.fin_len = a.take<int32_t>(R); p.is_fin = a.take<int32_t>(R);
    p.can = a.take<int32_t>(B); p.last = a.take<int32_t>(B);
    p.go = a.take<int32_t>((size_t)max_len + 1);
    p.run_score = a.take<float>(R); p.fin_score = a.take<float>(R);
    p.go2 = go2_words ? a.take<int32_t>(go2_words) : nullptr;
    const size_t H = rec ? 2 * R * max_len : 0;
    p.run_ts = H ? a.take<float>(H) : nullptr; p.run_tl = H ? a.take<float>(H) : nullptr;
    p.fin_ts = H ? a.take<float>(H) : nullptr; p.fin_tl = H ? a.take<float>(H) : nullptr;
    p.run_bi = H ? a.take<int32_t>(H) : nullptr; p.fin_bi = H ? a.take<int32_t>(H) : nullptr;
    p.marks = mark_bytes ? a.take<uint8_t>(mark_bytes) : nullptr;
    return p;
}

__host__ __device__ inline bool goes_on(bool greedy, uint32_t w) { return greedy ? w != 0 : ((w & 0xffffu) != 0 && (w >> 16) != 0); }

// grid B: the state before step 0
__global__ __launch_bounds__(NT) void avsr_search_init_kernel(SearchPtrs p, int B, int K, int max_len, int greedy, int bos, int pad, int32_t* go2) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t R = (size_t)B * K;
    for (int i = tid; i < K * max_len; i += NT) {
        const int tokv = (i % max_len) == 0 ? bos : pad;
        for (int par = 0; par < 2; ++par) {
            p.run_seq[((size_t)par * R + (size_t)b * K) * max_len + i] = tokv;
            p.fin_seq[((size_t)par * R + (size_t)b * K) * max_len + i] = tokv;
            if (p.run_ts) {
                const size_t at = ((size_t)par * R + (size_t)b * K) * max_len + i;
                p.run_ts[at] = 0.0f; p.run_tl[at] = 0.0f; p.fin_ts[at] = 0.0f; p.fin_tl[at] = 0.0f;
                p.run_bi[at] = -1; p.fin_bi[at] = -1;
            }
        }
    }
    if (tid < K) {
        const int r = b * K + tid;
        p.tok[r] = bos;
        p.src[r] = r;
        p.run_score[r] = tid == 0 ? 0.0f : -1.0e9f;
        p.fin_score[r] = -1.0e9f;
        p.fin_len[r] = greedy ? 1 : 0;
        p.is_fin[r] = 0;
    }
    if (tid == 0) { p.can[b] = 1; p.last[b] = 0; }
    if (b == 0)
        for (int i = tid; i <= max_len; i += NT) {
            p.go[i] = i == 0 ? (greedy ? B : 0x10001) : 0;
            if (go2) go2[i] = i == 0 ? 1 : 0;
        }
}

// (value, index) maximum, equal values: the lower index — over the 256 threads of a workgroup; every thread returns the result
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sv, int* si) {
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();                                     // the previous use of sv / si has been read by everyone
    if ((threadIdx.x & 63) == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int k = 1; k < NT / 64; ++k)
        if (sv[k] > v || (sv[k] == v && si[k] < i)) { v = sv[k]; i = si[k]; }
}

// the marks of `rows` hypothesis rows (the file's head comment): marks [rows][Vp] bytes, seq [rows][max_len] holds positions 0 .. step
__device__ void build_marks(uint8_t* marks, const int32_t* seq, int rows, int max_len, int V, int Vp, int step, int eos, const OptArgs& o) {
    const int tid = threadIdx.x, n = o.ngram;
    uint32_t* words = reinterpret_cast<uint32_t*>(marks);
    for (int i = tid; i < rows * (Vp / 4); i += NT) words[i] = 0u;
    __syncthreads();
    for (int k = 0; k < rows; ++k)
        for (int pos = tid; pos <= step; pos += NT) {
            const int t = seq[(size_t)k * max_len + pos];
            if ((unsigned)t < (unsigned)V) marks[(size_t)k * Vp + t] = 1;
        }
    __syncthreads();
    if (n > 0 && step + 1 >= n)                          // windows [i, i + n) of the prefix whose first n - 1 tokens equal its last n - 1
        for (int k = 0; k < rows; ++k) {
            const int32_t* sq = seq + (size_t)k * max_len;
            for (int i = tid; i + n - 1 <= step; i += NT) {
                bool match = true;
                for (int j = 0; j < n - 1 && match; ++j) match = sq[i + j] == sq[step + 2 - n + j];
                const int t = sq[i + n - 1];
                if (match && (unsigned)t < (unsigned)V) marks[(size_t)k * Vp + t] = 2;
            }
        }
    if (step < o.min_new && tid < rows && (unsigned)eos < (unsigned)V) marks[(size_t)tid * Vp + eos] = 2;
    __syncthreads();
}

__device__ __forceinline__ float processed(float s, uint8_t mark, float penalty) {
    if (mark == 1) s = s < 0.0f ? s * penalty : s / penalty;
    return mark == 2 ? -INFINITY : s;
}

// grid B (rows): transformers' _sample with do_sample False for one step.  REC: the chosen token's processed logit and the row's
// log-sum-exp go to run_ts / run_tl (one copy: greedy rows are never re-parented), the processed row to dump (if not null)
template <bool OPTS, bool REC>
__global__ __launch_bounds__(NT) void avsr_greedy_step_kernel(const float* __restrict__ logits, int V, int Vp, int step, int max_len, int eos, int pad,
                                                              SearchPtrs p, OptArgs o, float* __restrict__ dump) {
    extern __shared__ __align__(16) uint8_t lds_marks[];
    __shared__ float sv[NT / 64];
    __shared__ int si[NT / 64];
    if (p.go[step] == 0) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (size_t)b * Vp;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if constexpr (OPTS) {
        uint8_t* marks = o.marks ? o.marks + (size_t)b * Vp : lds_marks;
        build_marks(marks, p.run_seq + (size_t)b * max_len, 1, max_len, V, Vp, step, eos, o);
        for (int v = tid; v < V; v += NT) {
            const float x = processed(row[v], marks[v], o.penalty);
            if (x > best) { best = x; bi = v; }
        }
    } else {
        for (int v = tid; v < V; v += NT) {
            const float x = row[v];
            if (x > best) { best = x; bi = v; }
        }
    }
    block_argmax(best, bi, sv, si);
    float lse = 0.0f;
    if constexpr (REC) {                                  // Z in the file's documented order; best is M
        __shared__ float zred[NT];
        float z = 0.0f;
        for (int v = tid; v < V; v += NT) {
            float x = row[v];
            if constexpr (OPTS) x = processed(x, (o.marks ? o.marks + (size_t)b * Vp : lds_marks)[v], o.penalty);
            z += x == -INFINITY ? 0.0f : rs_expf(x - best);
            if (dump) dump[(size_t)b * Vp + v] = x;
        }
        if (dump)
            for (int v = V + tid; v < Vp; v += NT) dump[(size_t)b * Vp + v] = 0.0f;
        zred[tid] = z;
        __syncthreads();
        for (int stride = NT / 2; stride > 0; stride >>= 1) {
            if (tid < stride) zred[tid] += zred[tid + stride];
            __syncthreads();
        }
        lse = best == -INFINITY ? -INFINITY : best + rs_logf(zred[0]);
    }
    if (tid == 0) {
        if (bi >= V) bi = 0;
        const int unfinished = p.can[b];
        if constexpr (REC)
            if (unfinished) {
                p.run_ts[(size_t)b * max_len + step + 1] = best;
                p.run_tl[(size_t)b * max_len + step + 1] = lse;
            }
        const int nxt = unfinished ? bi : pad;
        p.run_seq[(size_t)b * max_len + step + 1] = nxt;
        p.tok[b] = nxt;
        if (unfinished) p.fin_len[b] = step + 2;
        const int still = unfinished && nxt != eos;
        p.can[b] = still;
        p.last[b] = step + 1;
        if (still) atomicAdd(&p.go[step + 1], 1);
    }
}

// grid B (clips): transformers' _beam_search for one step (the file's head comment).  REC: RECORDING there
template <bool OPTS, bool REC>
__global__ __launch_bounds__(NT) void avsr_beam_step_kernel(const float* __restrict__ logits, int V, int Vp, int K, int step, int max_len, int eos, float den,
                                                            float den_heur, int B, SearchPtrs p, OptArgs o, float* __restrict__ dump) {
    extern __shared__ __align__(16) uint8_t lds_marks[];
    __shared__ float red[MAXK][NT];
    __shared__ float row_max[MAXK], row_lse[MAXK], row_run[MAXK];
    __shared__ float top_lp[2 * MAXK], lp_run[2 * MAXK], m_score[3 * MAXK], new_score[MAXK];
    __shared__ int top_idx[2 * MAXK], parent[2 * MAXK], token[2 * MAXK], ends[2 * MAXK], just[2 * MAXK];
    __shared__ int keep[MAXK], best[MAXK], old_len[MAXK], old_fin[MAXK], used[3 * MAXK];
    __shared__ float sv[NT / 64];
    __shared__ int si[NT / 64];
    __shared__ float row_pmax[REC ? MAXK : 1], row_plse[REC ? MAXK : 1], cand_ts[REC ? 2 * MAXK : 1], cand_tl[REC ? 2 * MAXK : 1];
    if (!goes_on(false, (uint32_t)p.go[step])) return;
    if constexpr (OPTS)
        if (o.go2 && o.go2[step] == 0) return;
    const int b = blockIdx.x, tid = threadIdx.x, cur = step + 1;
    const size_t R = (size_t)B * K;
    const float* lg = logits + (size_t)b * K * Vp;
    const uint8_t* marks = nullptr;
    if constexpr (OPTS) {
        uint8_t* mk = o.marks ? o.marks + (size_t)b * K * Vp : lds_marks;
        build_marks(mk, p.run_seq + ((size_t)(step & 1) * R + (size_t)b * K) * max_len, K, max_len, V, Vp, step, eos, o);
        marks = mk;
    }

    // 1. per-row maximum and sum of exponentials
    for (int k = 0; k < K; ++k) {
        float m = -INFINITY;
        for (int v = tid; v < V; v += NT) m = fmaxf(m, lg[(size_t)k * Vp + v]);
        red[k][tid] = m;
    }
    if (tid < K) row_run[tid] = p.run_score[b * K + tid];
    __syncthreads();
    for (int stride = NT / 2; stride > 0; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < K; ++k) red[k][tid] = fmaxf(red[k][tid], red[k][tid + stride]);
        __syncthreads();
    }
    if (tid < K) row_max[tid] = red[tid][0];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const float m = row_max[k];
        float s = 0.0f;
        for (int v = tid; v < V; v += NT) s += rs_expf(lg[(size_t)k * Vp + v] - m);
        red[k][tid] = s;
    }
    __syncthreads();
    for (int stride = NT / 2; stride > 0; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + stride];
        __syncthreads();
    }
    if (tid < K) row_lse[tid] = rs_logf(red[tid][0]);
    __syncthreads();

    if constexpr (REC) {                                  // 1b. per row: maximum M and log-sum-exp of the processed scores (RECORDING)
        for (int k = 0; k < K; ++k) {
            const float m = row_max[k], l = row_lse[k];
            float pm = -INFINITY;
            for (int v = tid; v < V; v += NT) {
                float s = (lg[(size_t)k * Vp + v] - m) - l;
                if constexpr (OPTS) s = processed(s, marks[(size_t)k * Vp + v], o.penalty);
                pm = fmaxf(pm, s);
                if (dump) dump[((size_t)b * K + k) * Vp + v] = s;
            }
            if (dump)
                for (int v = V + tid; v < Vp; v += NT) dump[((size_t)b * K + k) * Vp + v] = 0.0f;
            red[k][tid] = pm;
        }
        __syncthreads();
        for (int stride = NT / 2; stride > 0; stride >>= 1) {
            if (tid < stride)
                for (int k = 0; k < K; ++k) red[k][tid] = fmaxf(red[k][tid], red[k][tid + stride]);
            __syncthreads();
        }
        if (tid < K) row_pmax[tid] = red[tid][0];
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const float m = row_max[k], l = row_lse[k], M = row_pmax[k];
            float z = 0.0f;
            for (int v = tid; v < V; v += NT) {
                float s = (lg[(size_t)k * Vp + v] - m) - l;
                if constexpr (OPTS) s = processed(s, marks[(size_t)k * Vp + v], o.penalty);
                z += s == -INFINITY ? 0.0f : rs_expf(s - M);
            }
            red[k][tid] = z;
        }
        __syncthreads();
        for (int stride = NT / 2; stride > 0; stride >>= 1) {
            if (tid < stride)
                for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + stride];
            __syncthreads();
        }
        if (tid < K) row_plse[tid] = row_pmax[tid] == -INFINITY ? -INFINITY : row_pmax[tid] + rs_logf(red[tid][0]);
        __syncthreads();
    }

    // 2. the 2 K best (value descending, flat index ascending)
    float prev_v = INFINITY;
    int prev_i = -1;
    for (int r = 0; r < 2 * K; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = 0; k < K; ++k) {
            const float m = row_max[k], lse = row_lse[k], run = row_run[k];
            for (int v = tid; v < V; v += NT) {
                float val = (lg[(size_t)k * Vp + v] - m) - lse;
                if constexpr (OPTS) val = processed(val, marks[(size_t)k * Vp + v], o.penalty);
                val = val + run;
                const int idx = k * V + v;
                const bool after = val < prev_v || (val == prev_v && idx > prev_i);
                if (after && (val > bv || (val == bv && idx < bi))) { bv = val; bi = idx; }
            }
        }
        block_argmax(bv, bi, sv, si);
        if (tid == 0) { top_lp[r] = bv; top_idx[r] = bi; }
        prev_v = bv; prev_i = bi;
    }
    __syncthreads();

    // 3. bookkeeping (generation.py's lines in float32, in its order)
    if (tid == 0) {
        const float NEG = -1.0e9f;
        const int ci = p.can[b];
        int all_end = 1;
        for (int j = 0; j < 2 * K; ++j) {
            int idx = top_idx[j];
            if (idx < 0 || idx >= K * V) idx = 0;        // only if a row held NaN: stay inside the buffers
            parent[j] = idx / V; token[j] = idx % V;
            ends[j] = (token[j] == eos) || (cur + 1 >= max_len);
            all_end &= ends[j];
            lp_run[j] = top_lp[j] + (ends[j] ? 1.0f : 0.0f) * NEG;
            used[j] = 0;
            if constexpr (REC) {                          // the selection's own value before the running score was added
                float s = (lg[(size_t)parent[j] * Vp + token[j]] - row_max[parent[j]]) - row_lse[parent[j]];
                if constexpr (OPTS) s = processed(s, marks[(size_t)parent[j] * Vp + token[j]], o.penalty);
                cand_ts[j] = s; cand_tl[j] = row_plse[parent[j]];
            }
        }
        for (int j = 0; j < K; ++j) {                     // stable: the first of equal values
            int w = -1;
            for (int c = 0; c < 2 * K; ++c)
                if (!used[c] && (w < 0 || lp_run[c] > lp_run[w])) w = c;
            used[w] = 1; keep[j] = w;
        }
        for (int j = 0; j < K; ++j) {
            m_score[j] = p.fin_score[b * K + j];
            old_len[j] = p.fin_len[b * K + j];
            old_fin[j] = p.is_fin[b * K + j];
        }
        int full = 0;                                     // early_stopping True: all K slots were finished before this step
        if constexpr (OPTS) {
            full = o.es_true;
            for (int j = 0; j < K; ++j) full &= old_fin[j] != 0;
        }
        for (int j = 0; j < 2 * K; ++j) {
            just[j] = ends[j] && j < K;
            float f = top_lp[j] / den;
            if constexpr (OPTS) f = f + (full ? 1.0f : 0.0f) * NEG;
            f = f + (ci ? 0.0f : 1.0f) * NEG;
            f = f + (just[j] ? 0.0f : 1.0f) * NEG;
            m_score[K + j] = f;
        }
        for (int c = 0; c < 3 * K; ++c) used[c] = 0;
        for (int j = 0; j < K; ++j) {
            int w = -1;
            for (int c = 0; c < 3 * K; ++c)
                if (!used[c] && (w < 0 || m_score[c] > m_score[w])) w = c;
            used[w] = 1; best[j] = w;
        }
        float mn = INFINITY;
        for (int j = 0; j < K; ++j) {
            const int w = best[j];
            new_score[j] = m_score[w];
            mn = fminf(mn, m_score[w]);
        }
        const float best_running = lp_run[keep[0]] / den_heur;
        int any = 0, all_fin = 1;
        for (int j = 0; j < K; ++j) {
            const int w = best[j];
            const int nf = w < K ? old_fin[w] : just[w - K];
            all_fin &= nf != 0;
            p.fin_score[b * K + j] = new_score[j];
            p.fin_len[b * K + j] = w < K ? old_len[w] : cur + 1;
            p.is_fin[b * K + j] = nf;
            any |= best_running > (nf ? mn : NEG);
        }
        for (int j = 0; j < K; ++j) {
            p.run_score[b * K + j] = lp_run[keep[j]];
            p.tok[b * K + j] = token[keep[j]];
            p.src[b * K + j] = b * K + parent[keep[j]];
        }
        const int ci_new = ci && any;
        p.can[b] = ci_new;
        p.last[b] = cur;
        atomicAdd(&p.go[cur], (ci_new ? 1 : 0) + (all_end ? 0 : 0x10000));
        if constexpr (OPTS)
            if (o.go2 && !all_fin) atomicAdd(&o.go2[cur], 1);
    }
    __syncthreads();
    const int32_t* run_s = p.run_seq + ((size_t)(step & 1) * R + (size_t)b * K) * max_len;
    const int32_t* fin_s = p.fin_seq + ((size_t)(step & 1) * R + (size_t)b * K) * max_len;
    int32_t* run_d = p.run_seq + ((size_t)(cur & 1) * R + (size_t)b * K) * max_len;
    int32_t* fin_d = p.fin_seq + ((size_t)(cur & 1) * R + (size_t)b * K) * max_len;
    for (int j = 0; j < K; ++j) {
        const int c = keep[j], w = best[j];
        for (int pos = tid; pos <= cur && pos < max_len; pos += NT) {
            run_d[(size_t)j * max_len + pos] = pos == cur ? token[c] : run_s[(size_t)parent[c] * max_len + pos];
            int32_t f;
            if (w < K) f = fin_s[(size_t)w * max_len + pos];
            else f = pos == cur ? token[w - K] : run_s[(size_t)parent[w - K] * max_len + pos];
            fin_d[(size_t)j * max_len + pos] = f;
        }
    }
    if constexpr (REC) {                                  // the histories follow the prefixes: same parity, same re-parenting
        const size_t src_o = ((size_t)(step & 1) * R + (size_t)b * K) * max_len, dst_o = ((size_t)(cur & 1) * R + (size_t)b * K) * max_len;
        for (int j = 0; j < K; ++j) {
            const int c = keep[j], w = best[j];
            for (int pos = 1 + tid; pos <= cur && pos < max_len; pos += NT) {
                const size_t rp = src_o + (size_t)parent[c] * max_len + pos, d = dst_o + (size_t)j * max_len + pos;
                p.run_ts[d] = pos == cur ? cand_ts[c] : p.run_ts[rp];
                p.run_tl[d] = pos == cur ? cand_tl[c] : p.run_tl[rp];
                p.run_bi[d] = pos == cur ? b * K + parent[c] : p.run_bi[rp];
                if (w < K) {
                    const size_t fp = src_o + (size_t)w * max_len + pos;
                    p.fin_ts[d] = p.fin_ts[fp]; p.fin_tl[d] = p.fin_tl[fp]; p.fin_bi[d] = p.fin_bi[fp];
                } else {
                    const int cw = w - K;
                    const size_t wp = src_o + (size_t)parent[cw] * max_len + pos;
                    p.fin_ts[d] = pos == cur ? cand_ts[cw] : p.run_ts[wp];
                    p.fin_tl[d] = pos == cur ? cand_tl[cw] : p.run_tl[wp];
                    p.fin_bi[d] = pos == cur ? b * K + parent[cw] : p.run_bi[wp];
                }
            }
        }
    }
}

// grid B: the result of clip b: its n_ret best finished hypotheses (beam; slots 0 .. n_ret - 1, output rows b n_ret + j) or its row
// (greedy, n_ret 1), from the buffers the last step wrote
__global__ __launch_bounds__(NT) void avsr_search_finish_kernel(SearchPtrs p, int B, int K, int max_len, int greedy, int n_ret, int32_t* sequences,
                                                                int32_t* lengths, float* scores) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t R = (size_t)B * K;
    const int n = p.last[b];
    const int32_t* src = greedy ? p.run_seq + (size_t)b * max_len : p.fin_seq + ((size_t)(n & 1) * R + (size_t)b * K) * max_len;
    for (int i = tid; i < n_ret * max_len; i += NT) sequences[(size_t)b * n_ret * max_len + i] = src[i];
    if (tid < n_ret) {
        lengths[b * n_ret + tid] = p.fin_len[(size_t)b * K + tid];
        if (scores) scores[b * n_ret + tid] = greedy ? 0.0f : p.fin_score[(size_t)b * K + tid];
    }
}

// grid B, after avsr_search_finish_kernel: the recorded histories of the same rows, [B n_ret][max_len - 1] (RECORDING); steps: last[0]
__global__ __launch_bounds__(NT) void avsr_search_finish_scored_kernel(SearchPtrs p, int B, int K, int max_len, int greedy, int n_ret,
                                                                       float* __restrict__ token_scores, float* __restrict__ token_lse,
                                                                       int32_t* __restrict__ beam_indices, int32_t* __restrict__ steps) {
    const int b = blockIdx.x, tid = threadIdx.x, N = max_len - 1;
    const size_t R = (size_t)B * K;
    const size_t at = greedy ? (size_t)b * max_len : ((size_t)(p.last[b] & 1) * R + (size_t)b * K) * max_len;
    const float *ts = (greedy ? p.run_ts : p.fin_ts) + at, *tl = (greedy ? p.run_tl : p.fin_tl) + at;
    const int32_t* bi = p.fin_bi + at;
    for (int i = tid; i < n_ret * N; i += NT) {
        const int j = i / N, pos = i % N + 1;
        const bool live = pos < p.fin_len[(size_t)b * K + j];
        const size_t o = (size_t)b * n_ret * N + i, h = (size_t)j * max_len + pos;
        token_scores[o] = live ? ts[h] : 0.0f;
        token_lse[o] = live ? tl[h] : 0.0f;
        if (beam_indices) beam_indices[o] = live && !greedy ? bi[h] : -1;
    }
    if (b == 0 && tid == 0 && steps) *steps = p.last[0];
}

// the options of a call: neutral for a null pointer; what the kernels and the state layout need of them
struct Opts {
    rs_avsr_search_opts o{1.0f, 0, 0, 0, 1};
    bool rec = false;           // the _scored entry points: the histories are part of the state
    bool kernel() const { return o.repetition_penalty != 1.0f || o.no_repeat_ngram_size > 0 || o.min_new_tokens > 0 || o.early_stopping == 1; }
    bool es_true() const { return o.early_stopping == 1; }
};
size_t mark_bytes(bool opts_kernel, int B, int K, int vocab) {       // marks kept in the state: only where a clip's K rows exceed the LDS share
    const size_t Vp = (size_t)(vocab + 3) / 4 * 4;
    return opts_kernel && (size_t)K * Vp > (size_t)MARK_LDS_BYTES ? (size_t)B * K * Vp : 0;
}
SearchPtrs search_layout_opts(const Opts& op, int B, int K, int max_len, int vocab, rs_arena& a) {
    return search_layout(B, K, max_len, op.es_true() ? (size_t)max_len + 1 : 0, mark_bytes(op.kernel(), B, K, vocab), op.rec, a);
}
size_t search_bytes(const Opts& op, int B, int K, int max_len, int vocab) {
    rs_arena a;
    search_layout_opts(op, B, K, max_len, vocab, a);
    return a.bytes() + SEARCH_SLACK;
}
OptArgs opt_args(const Opts& op, const SearchPtrs& p) {      // (go2 / marks are null where the layout did not take them)
    OptArgs a;
    a.penalty = op.o.repetition_penalty; a.ngram = op.o.no_repeat_ngram_size; a.min_new = op.o.min_new_tokens; a.es_true = op.es_true() ? 1 : 0;
    a.go2 = p.go2;
    a.marks = p.marks;
    return a;
}

// the arguments of a search call -> its options.  vocab 0: a call that touches the front of the state only (rows, peek, finish)
int check_search_args(rs_ctx* ctx, const rs_avsr_search* sp, const rs_avsr_search_opts* opts, int B, int vocab, const void* state, const char* what, Opts* op) {
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);        // (the entry's guard: an avsr context)
    if (!sp || !state) return rs_fail(ctx, RS_EINVAL, "%s: null pointer", what);
    if (sp->beams < 1 || sp->beams > MAXK) return rs_fail(ctx, RS_EINVAL, "%s: beams must be 1..%d, got %d", what, MAXK, sp->beams);
    if (sp->greedy && sp->beams != 1) return rs_fail(ctx, RS_EINVAL, "%s: greedy search has one row per clip, got beams %d", what, sp->beams);
    if (sp->max_new_tokens < 1) return rs_fail(ctx, RS_EINVAL, "%s: max_new_tokens %d", what, sp->max_new_tokens);
    if (1 + (long long)sp->max_new_tokens > d->max_positions)
        return rs_fail(ctx, RS_EINVAL, "%s: 1 + max_new_tokens = %lld positions exceed max_target_positions %d", what, 1 + (long long)sp->max_new_tokens, d->max_positions);
    if (B <= 0 || B > 32767) return rs_fail(ctx, RS_EINVAL, "%s: %d clips (1 .. 32767)", what, B);
    const bool front = vocab == 0;
    if (!front && (vocab < 4 || (long long)vocab * sp->beams > 0x7fffffffLL)) return rs_fail(ctx, RS_EINVAL, "%s: vocabulary %d (at least 4)", what, vocab);
    if (opts) {
        op->o = *opts;
        if (!(opts->repetition_penalty > 0.0f)) return rs_fail(ctx, RS_EINVAL, "%s: repetition_penalty must be > 0, got %g", what, (double)opts->repetition_penalty);
        if (opts->no_repeat_ngram_size < 0 || opts->min_new_tokens < 0)
            return rs_fail(ctx, RS_EINVAL, "%s: no_repeat_ngram_size %d / min_new_tokens %d must not be negative", what, opts->no_repeat_ngram_size, opts->min_new_tokens);
        if (opts->early_stopping < 0 || opts->early_stopping > 2) return rs_fail(ctx, RS_EINVAL, "%s: early_stopping %d (0 False, 1 True, 2 never)", what, opts->early_stopping);
        if (opts->num_return_sequences < 1 || opts->num_return_sequences > sp->beams)
            return rs_fail(ctx, RS_EINVAL, "%s: num_return_sequences %d outside 1..beams (%d)", what, opts->num_return_sequences, sp->beams);
        if (sp->greedy && opts->num_return_sequences > 1) return rs_fail(ctx, RS_EINVAL, "%s: greedy search returns one sequence per clip, got num_return_sequences %d", what, opts->num_return_sequences);
        if (sp->greedy) op->o.early_stopping = 0;          // a beam-search switch: _sample never reads it
    }
    return RS_OK;
}
// the arguments, then the state carved: for a front-only call (vocab 0) the marks do not count towards the size it needs
int check_search(rs_ctx* ctx, const rs_avsr_search* sp, const rs_avsr_search_opts* opts, int B, int vocab, void* state, size_t state_bytes,
                 const char* what, SearchPtrs* p, Opts* op) {
    const int rc = check_search_args(ctx, sp, opts, B, vocab, state, what, op);
    if (rc != RS_OK) return rc;
    rs_arena arena(state);
    *p = search_layout_opts(*op, B, sp->beams, 1 + sp->max_new_tokens, vocab == 0 ? 4 : vocab, arena);
    if (state_bytes < arena.bytes() + SEARCH_SLACK) return rs_fail(ctx, RS_EWORKSPACE, "%s: state %zu < %zu", what, state_bytes, arena.bytes() + SEARCH_SLACK);
    return RS_OK;
}

bool opts_ok_for_bytes(const rs_avsr_search_opts* o, int beams) {
    return !o || (o->repetition_penalty > 0.0f && o->no_repeat_ngram_size >= 0 && o->min_new_tokens >= 0 && o->early_stopping >= 0 && o->early_stopping <= 2 &&
                  o->num_return_sequences >= 1 && o->num_return_sequences <= beams);
}

// ---- the entry points: every family (plain, _opts, _scored) is one implementation with the options and the recording as arguments ----
size_t search_state_bytes(const rs_ctx* ctx, int B, int beams, int max_len, int vocab, const rs_avsr_search_opts* opts, bool rec) {
    if (B <= 0 || beams < 1 || beams > MAXK || max_len < 2 || vocab < 4 || !opts_ok_for_bytes(opts, beams)) return 0;
    Opts op;
    op.rec = rec;
    if (opts) op.o = *opts;
    return search_bytes(op, B, beams, max_len, vocab);
}

int search_begin(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, bool rec, int B, int vocab, void* state, size_t state_bytes,
                 void* stream) {
    SearchPtrs p;
    Opts op;
    op.rec = rec;
    const int rc = check_search(ctx, search, opts, B, vocab, state, state_bytes, "rs_avsr_search_begin", &p, &op);
    if (rc != RS_OK) return rc;
    hipLaunchKernelGGL(avsr_search_init_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, p, B, search->beams, 1 + search->max_new_tokens,
                       search->greedy ? 1 : 0, search->bos_token_id, search->pad_token_id, p.go2);
    RS_CHECK_LAUNCH(ctx, "avsr search begin");
    return RS_OK;
}

// step_scores (rec only): f32[max_new_tokens][B * beams][Vp] or null
int search_step(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, const rs_avsr_search_opts* opts, bool rec, float* step_scores, int B,
                int vocab, void* state, size_t state_bytes, void* stream) {
    SearchPtrs p;
    Opts op;
    op.rec = rec;
    const int rc = check_search(ctx, search, opts, B, vocab, state, state_bytes, "rs_avsr_search_step", &p, &op);
    if (rc != RS_OK) return rc;
    if (!logits || step < 0 || step >= search->max_new_tokens) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_step: bad argument (step %d of %d)", step, search->max_new_tokens);
    const int max_len = 1 + search->max_new_tokens, Vp = (vocab + 3) / 4 * 4;
    const OptArgs oa = opt_args(op, p);
    const bool ok = op.kernel();
    // the marks of a workgroup's rows: dynamic LDS unless they live in the state
    const size_t lds = ok && !oa.marks ? (size_t)(search->greedy ? 1 : search->beams) * Vp : 0;
    float* const dump = rec && step_scores ? step_scores + (size_t)step * B * search->beams * Vp : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (search->greedy) {
#define RS_GREEDY(O, R) \
    hipLaunchKernelGGL((avsr_greedy_step_kernel<O, R>), dim3(B), dim3(NT), lds, s, logits, vocab, Vp, step, max_len, search->eos_token_id, search->pad_token_id, p, oa, dump)
        if (rec) { if (ok) RS_GREEDY(true, true); else RS_GREEDY(false, true); }
        else { if (ok) RS_GREEDY(true, false); else RS_GREEDY(false, false); }
#undef RS_GREEDY
    } else {
        const float den = (float)pow((double)(step + 1), (double)search->length_penalty);
        const float den_heur = op.o.early_stopping == 2 && search->length_penalty > 0.0f ? (float)pow((double)search->max_new_tokens, (double)search->length_penalty) : den;
#define RS_BEAM(O, R) \
    hipLaunchKernelGGL((avsr_beam_step_kernel<O, R>), dim3(B), dim3(NT), lds, s, logits, vocab, Vp, search->beams, step, max_len, search->eos_token_id, den, den_heur, B, p, oa, dump)
        if (rec) { if (ok) RS_BEAM(true, true); else RS_BEAM(false, true); }
        else { if (ok) RS_BEAM(true, false); else RS_BEAM(false, false); }
#undef RS_BEAM
    }
    RS_CHECK_LAUNCH(ctx, "avsr search step");
    return RS_OK;
}

int search_peek(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, bool rec, int B, void* state, size_t state_bytes, int step,
                int32_t* tokens, int32_t* src_rows, float* run_scores, float* fin_scores, int32_t* goes_on_out, void* stream) {
    SearchPtrs p;
    Opts op;
    op.rec = rec;
    const int rc = check_search(ctx, search, opts, B, 0, state, state_bytes, "rs_avsr_search_peek", &p, &op);
    if (rc != RS_OK) return rc;
    if (step < 0 || step > search->max_new_tokens) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_peek: step %d of %d", step, search->max_new_tokens);
    const size_t R = (size_t)B * search->beams;
    hipStream_t s = (hipStream_t)stream;
    uint32_t w = 0, w2 = 1;
    if (tokens) RS_HIP(ctx, hipMemcpyAsync(tokens, p.tok, R * 4, hipMemcpyDeviceToHost, s));
    if (src_rows) RS_HIP(ctx, hipMemcpyAsync(src_rows, p.src, R * 4, hipMemcpyDeviceToHost, s));
    if (run_scores) RS_HIP(ctx, hipMemcpyAsync(run_scores, p.run_score, R * 4, hipMemcpyDeviceToHost, s));
    if (fin_scores) RS_HIP(ctx, hipMemcpyAsync(fin_scores, p.fin_score, R * 4, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipMemcpyAsync(&w, p.go + step, 4, hipMemcpyDeviceToHost, s));
    if (op.es_true()) RS_HIP(ctx, hipMemcpyAsync(&w2, p.go2 + step, 4, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    if (goes_on_out) *goes_on_out = goes_on(search->greedy != 0, w) && w2 != 0 ? 1 : 0;
    return RS_OK;
}

// the recorded outputs of a _scored call; beam_indices may be null for a greedy search, steps always
struct ScoredOut { float *token_scores, *token_lse; int32_t *beam_indices, *steps; };
bool scored_out_ok(const rs_avsr_search* search, const ScoredOut& so) { return so.token_scores && so.token_lse && (so.beam_indices || search->greedy); }

int search_finish(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, const ScoredOut* so, int B, void* state, size_t state_bytes,
                  int32_t* sequences, int32_t* lengths, float* scores, void* stream) {
    SearchPtrs p;
    Opts op;
    op.rec = so != nullptr;
    const int rc = check_search(ctx, search, opts, B, 0, state, state_bytes, "rs_avsr_search_finish", &p, &op);
    if (rc != RS_OK) return rc;
    if (!sequences || !lengths || (so && !scored_out_ok(search, *so))) return rs_fail(ctx, RS_EINVAL, "rs_avsr_search_finish: null pointer");
    hipLaunchKernelGGL(avsr_search_finish_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, p, B, search->beams, 1 + search->max_new_tokens,
                       search->greedy ? 1 : 0, op.o.num_return_sequences, sequences, lengths, scores);
    RS_CHECK_LAUNCH(ctx, "avsr search finish");
    if (so) {
        hipLaunchKernelGGL(avsr_search_finish_scored_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, p, B, search->beams, 1 + search->max_new_tokens,
                           search->greedy ? 1 : 0, op.o.num_return_sequences, so->token_scores, so->token_lse, so->beam_indices, so->steps);
        RS_CHECK_LAUNCH(ctx, "avsr search finish (recorded scores)");
    }
    RS_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return RS_OK;
}

}  // namespace

extern "C" size_t rs_avsr_search_state_bytes_opts(const rs_ctx* ctx, int B, int beams, int max_len, int vocab, const rs_avsr_search_opts* opts) {
    RS_GUARD_QUERY(ctx, rs_avsr_search_state_bytes_opts, 0);
    return search_state_bytes(ctx, B, beams, max_len, vocab, opts, false);
}
extern "C" size_t rs_avsr_search_state_bytes_scored(const rs_ctx* ctx, int B, int beams, int max_len, int vocab, const rs_avsr_search_opts* opts) {
    RS_GUARD_QUERY(ctx, rs_avsr_search_state_bytes_scored, 0);
    return search_state_bytes(ctx, B, beams, max_len, vocab, opts, true);
}
extern "C" size_t rs_avsr_search_state_bytes(const rs_ctx* ctx, int B, int beams, int max_len) {
    RS_GUARD_QUERY(ctx, rs_avsr_search_state_bytes, 0);
    return rs_avsr_search_state_bytes_opts(ctx, B, beams, max_len, 4, nullptr);
}

extern "C" int rs_avsr_search_begin_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, int vocab, void* state,
                                         size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_begin_opts);
    return search_begin(ctx, search, opts, false, B, vocab, state, state_bytes, stream);
}
extern "C" int rs_avsr_search_begin_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, int vocab, void* state,
                                           size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_begin_scored);
    return search_begin(ctx, search, opts, true, B, vocab, state, state_bytes, stream);
}
extern "C" int rs_avsr_search_begin(rs_ctx* ctx, const rs_avsr_search* search, int B, int vocab, void* state, size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_begin);
    return rs_avsr_search_begin_opts(ctx, search, nullptr, B, vocab, state, state_bytes, stream);
}

extern "C" int rs_avsr_search_step_opts(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B,
                                        int vocab, void* state, size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_step_opts);
    return search_step(ctx, logits, step, search, opts, false, nullptr, B, vocab, state, state_bytes, stream);
}
extern "C" int rs_avsr_search_step_scored(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, const rs_avsr_search_opts* opts,
                                          float* step_scores, int B, int vocab, void* state, size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_step_scored);
    return search_step(ctx, logits, step, search, opts, true, step_scores, B, vocab, state, state_bytes, stream);
}
extern "C" int rs_avsr_search_step(rs_ctx* ctx, const float* logits, int step, const rs_avsr_search* search, int B, int vocab, void* state, size_t state_bytes,
                                   void* stream) {
    RS_GUARD(ctx, rs_avsr_search_step);
    return rs_avsr_search_step_opts(ctx, logits, step, search, nullptr, B, vocab, state, state_bytes, stream);
}

extern "C" int rs_avsr_search_rows(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, const int32_t** tokens,
                                   const int32_t** src_rows) {
    RS_GUARD(ctx, rs_avsr_search_rows);
    SearchPtrs p;
    Opts op;
    const int rc = check_search(ctx, search, nullptr, B, 0, state, state_bytes, "rs_avsr_search_rows", &p, &op);
    if (rc != RS_OK) return rc;
    if (tokens) *tokens = p.tok;
    if (src_rows) *src_rows = p.src;
    return RS_OK;
}

extern "C" int rs_avsr_search_peek_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state, size_t state_bytes,
                                        int step, int32_t* tokens, int32_t* src_rows, float* run_scores, float* fin_scores, int32_t* goes_on_out, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_peek_opts);
    return search_peek(ctx, search, opts, false, B, state, state_bytes, step, tokens, src_rows, run_scores, fin_scores, goes_on_out, stream);
}
extern "C" int rs_avsr_search_peek_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state, size_t state_bytes,
                                          int step, int32_t* tokens, int32_t* src_rows, float* run_scores, float* fin_scores, int32_t* goes_on_out,
                                          void* stream) {
    RS_GUARD(ctx, rs_avsr_search_peek_scored);
    return search_peek(ctx, search, opts, true, B, state, state_bytes, step, tokens, src_rows, run_scores, fin_scores, goes_on_out, stream);
}
extern "C" int rs_avsr_search_peek(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int step, int32_t* tokens, int32_t* src_rows,
                                   float* run_scores, float* fin_scores, int32_t* goes_on_out, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_peek);
    return rs_avsr_search_peek_opts(ctx, search, nullptr, B, state, state_bytes, step, tokens, src_rows, run_scores, fin_scores, goes_on_out, stream);
}

extern "C" int rs_avsr_search_finish_opts(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state, size_t state_bytes,
                                          int32_t* sequences, int32_t* lengths, float* scores, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_finish_opts);
    return search_finish(ctx, search, opts, nullptr, B, state, state_bytes, sequences, lengths, scores, stream);
}
extern "C" int rs_avsr_search_finish_scored(rs_ctx* ctx, const rs_avsr_search* search, const rs_avsr_search_opts* opts, int B, void* state, size_t state_bytes,
                                            int32_t* sequences, int32_t* lengths, float* scores, float* token_scores, float* token_lse, int32_t* beam_indices,
                                            int32_t* steps_run, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_finish_scored);
    const ScoredOut so{token_scores, token_lse, beam_indices, steps_run};
    return search_finish(ctx, search, opts, &so, B, state, state_bytes, sequences, lengths, scores, stream);
}
extern "C" int rs_avsr_search_finish(rs_ctx* ctx, const rs_avsr_search* search, int B, void* state, size_t state_bytes, int32_t* sequences, int32_t* lengths,
                                     float* scores, void* stream) {
    RS_GUARD(ctx, rs_avsr_search_finish);
    return rs_avsr_search_finish_opts(ctx, search, nullptr, B, state, state_bytes, sequences, lengths, scores, stream);
}

// ---- generate(): decoder step + search step per token, the stop word read LAG steps behind ------------------------------------------
namespace {
// the decoder's state and the search's state as two pieces (each with its own layout and slack inside), then a step's logits
struct GenPlan { char *dec, *search; float* logits; size_t dec_bytes, search_bytes; };
constexpr size_t GEN_SLACK = 256;
GenPlan gen_plan(const rs_ctx* ctx, int B, int T, int beams, int max_len, const Opts& op, rs_arena& a) {
    GenPlan g{};
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);
    g.dec_bytes = rs_align(rs_avsr_decoder_state_bytes(ctx, B, T, beams, max_len));
    g.search_bytes = rs_align(search_bytes(op, B, beams, max_len, d->vocab_size));
    g.dec = a.take<char>(g.dec_bytes);
    g.search = a.take<char>(g.search_bytes);
    g.logits = a.take<float>((size_t)B * beams * ((d->vocab_size + 3) / 4 * 4));
    return g;
}
struct StopWatch {              // pinned words the go[] entries are copied to, and the events that say when they have arrived
    int32_t* words = nullptr;
    hipEvent_t ev[LAG + 1] = {};
    int n_ev = 0;
    ~StopWatch() {
        for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
        if (words) (void)hipHostFree(words);
    }
};

size_t generate_state_bytes(const rs_ctx* ctx, int B, int T, int beams, int max_len, const rs_avsr_search_opts* opts, bool rec) {
    if (B <= 0 || T <= 0 || beams < 1 || beams > MAXK || max_len < 2 || !opts_ok_for_bytes(opts, beams)) return 0;
    Opts op;
    op.rec = rec;
    if (opts) op.o = *opts;
    rs_arena a;
    gen_plan(ctx, B, T, beams, max_len, op, a);
    return a.bytes() + GEN_SLACK;
}
}  // namespace

extern "C" size_t rs_avsr_generate_state_bytes_opts(const rs_ctx* ctx, int B, int T, int beams, int max_len, const rs_avsr_search_opts* opts) {
    RS_GUARD_QUERY(ctx, rs_avsr_generate_state_bytes_opts, 0);
    return generate_state_bytes(ctx, B, T, beams, max_len, opts, false);
}
extern "C" size_t rs_avsr_generate_state_bytes_scored(const rs_ctx* ctx, int B, int T, int beams, int max_len, const rs_avsr_search_opts* opts) {
    RS_GUARD_QUERY(ctx, rs_avsr_generate_state_bytes_scored, 0);
    return generate_state_bytes(ctx, B, T, beams, max_len, opts, true);
}
extern "C" size_t rs_avsr_generate_state_bytes(const rs_ctx* ctx, int B, int T, int beams, int max_len) {
    RS_GUARD_QUERY(ctx, rs_avsr_generate_state_bytes, 0);
    return rs_avsr_generate_state_bytes_opts(ctx, B, T, beams, max_len, nullptr);
}

namespace {
// so null: nothing is recorded (the plain and _opts forms)
int generate(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search, const rs_avsr_search_opts* opts,
             const ScoredOut* so, float* step_scores, int32_t* sequences, int32_t* lengths, float* scores, void* state, size_t state_bytes, void* stream) {
    const rs_avsr_dims* d = rs_avsr_dims_of(ctx);
    if (!search || !enc || !padding_mask || !sequences || !lengths || !state || T <= 0 || (so && !scored_out_ok(search, *so)))
        return rs_fail(ctx, RS_EINVAL, "rs_avsr_generate: bad argument");
    const bool rec = so != nullptr;
    Opts op;
    op.rec = rec;
    int rc = check_search_args(ctx, search, opts, B, d->vocab_size, state, "rs_avsr_generate", &op);
    if (rc != RS_OK) return rc;
    const int K = search->beams, max_len = 1 + search->max_new_tokens;
    const bool greedy = search->greedy != 0, two_words = op.es_true();
    rs_arena arena(state);
    const GenPlan g = gen_plan(ctx, B, T, K, max_len, op, arena);
    if (state_bytes < arena.bytes() + GEN_SLACK) return rs_fail(ctx, RS_EWORKSPACE, "rs_avsr_generate: state %zu < %zu", state_bytes, arena.bytes() + GEN_SLACK);
    void *const dec_state = g.dec, *const s_state = g.search;
    float* const logits = g.logits;
    const size_t dec_bytes = g.dec_bytes, s_bytes = g.search_bytes;
    hipStream_t s = (hipStream_t)stream;
    rs_arena s_arena(s_state);
    const SearchPtrs p = search_layout_opts(op, B, K, max_len, d->vocab_size, s_arena);

    StopWatch sw;                // words[i]: go[i]; words[max_len + 1 + i]: go2[i] (early_stopping True)
    RS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&sw.words), (size_t)(max_len + 1) * 4 * 2, hipHostMallocDefault));
    for (; sw.n_ev < LAG + 1; ++sw.n_ev) RS_HIP(ctx, hipEventCreateWithFlags(&sw.ev[sw.n_ev], hipEventDisableTiming));

    rc = rs_avsr_decoder_begin(ctx, enc, B, T, K, max_len, dec_state, dec_bytes, stream);
    if (rc != RS_OK) return rc;
    rc = search_begin(ctx, search, opts, rec, B, d->vocab_size, s_state, s_bytes, stream);
    if (rc != RS_OK) return rc;
    for (int step = 0; step < search->max_new_tokens; ++step) {
        // greedy rows keep their caches (no re-parenting); beam rows are re-parented by the rows the last selection wrote
        rc = rs_avsr_decoder_step(ctx, p.tok, greedy ? nullptr : p.src, step, padding_mask, B, T, K, max_len, logits, dec_state, dec_bytes, stream);
        if (rc != RS_OK) return rc;
        rc = search_step(ctx, logits, step, search, opts, rec, step_scores, B, d->vocab_size, s_state, s_bytes, stream);
        if (rc != RS_OK) return rc;
        RS_HIP(ctx, hipMemcpyAsync(sw.words + step + 1, p.go + step + 1, 4, hipMemcpyDeviceToHost, s));
        if (two_words) RS_HIP(ctx, hipMemcpyAsync(sw.words + max_len + 1 + step + 1, p.go2 + step + 1, 4, hipMemcpyDeviceToHost, s));
        RS_HIP(ctx, hipEventRecord(sw.ev[step % (LAG + 1)], s));
        if (step >= LAG) {       // the word of step - LAG: steps issued past the stop return at once and change nothing
            const int e = step - LAG;
            RS_HIP(ctx, hipEventSynchronize(sw.ev[e % (LAG + 1)]));
            if (!goes_on(greedy, (uint32_t)sw.words[e + 1]) || (two_words && sw.words[max_len + 1 + e + 1] == 0)) break;
        }
    }
    return search_finish(ctx, search, opts, so, B, s_state, s_bytes, sequences, lengths, scores, stream);
}
}  // namespace

extern "C" int rs_avsr_generate_opts(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search,
                                     const rs_avsr_search_opts* opts, int32_t* sequences, int32_t* lengths, float* scores, void* state, size_t state_bytes,
                                     void* stream) {
    RS_GUARD(ctx, rs_avsr_generate_opts);
    return generate(ctx, enc, padding_mask, B, T, search, opts, nullptr, nullptr, sequences, lengths, scores, state, state_bytes, stream);
}
extern "C" int rs_avsr_generate_scored(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search,
                                       const rs_avsr_search_opts* opts, float* step_scores, int32_t* sequences, int32_t* lengths, float* scores,
                                       float* token_scores, float* token_lse, int32_t* beam_indices, int32_t* steps_run, void* state, size_t state_bytes,
                                       void* stream) {
    RS_GUARD(ctx, rs_avsr_generate_scored);
    const ScoredOut so{token_scores, token_lse, beam_indices, steps_run};
    return generate(ctx, enc, padding_mask, B, T, search, opts, &so, step_scores, sequences, lengths, scores, state, state_bytes, stream);
}
extern "C" int rs_avsr_generate(rs_ctx* ctx, const float* enc, const float* padding_mask, int B, int T, const rs_avsr_search* search, int32_t* sequences,
                                int32_t* lengths, float* scores, void* state, size_t state_bytes, void* stream) {
    RS_GUARD(ctx, rs_avsr_generate);
    return rs_avsr_generate_opts(ctx, enc, padding_mask, B, T, search, nullptr, sequences, lengths, scores, state, state_bytes, stream);
}
