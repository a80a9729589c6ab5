// k_rnnt_align.hip — forced alignment and transcript likelihood on the transducer lattice (rs_rnnt_align; Graves 2012).
// Given the labels y_1..y_U of utterance b (T frames), with g(u) the prediction network after the start context and the first u
// labels (u = 0..U), z(t,u) = W_out . act(f[b][t] + g(u)) + b_out, lb(t,u) = z[blank] - lse(z), ly(t,u) = z[y_(u+1)] - lse(z):
//   standard topology      a(0,0) = 0, a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t,u-1) + ly(t,u-1)),   loglik = a(T-1,U) + lb(T-1,U)
//   RS_ALIGN_ONE_PER_FRAME a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t-1,u-1) + ly(t-1,u-1)), t = 0..T, loglik = a(T,U)  (U <= T)
//   lae(a, b)              m = max(a, b); -inf when m is -inf, else m + rs_logf(rs_expf(a - m) + rs_expf(b - m)); a = the blank term
//   best                   the same recursion with max (ties to the blank predecessor); frames[b][u] = the frame at which label
//                          u + 1 is emitted on that path, logp[b][u] = ly(frames[b][u], u)
// Every number is float32 in one order, restated serially by tests/rnnt_align_checker.c, which the results equal bit for bit:
//   g, z, lse   exactly the routines of rs_rnnt_token_scores (k_rnnt_scores.hip): the lock-step LSTM chain over longest + 1 steps
//               (Zipformer: one stateless-decoder launch per chunk over its rows), rnnt_tile_kernel<4> over rows a_pre = act(f + g),
//               the lane-strided log-sum-exp of rnnt_logp_pick_kernel — so ly(t,u) is what token scores give for token u at frame t
//   the lattice the cells (b, t, u), t < T_b, u <= U_b, of the rows that have an alignment form one compacted list: utterance by
//               utterance, inside one by anti-diagonal d = t + u (outer) and u (inner), so the DP reads a diagonal coalesced.  The
//               list is scored in chunks of R rows (R a multiple of 32 that follows from the workspace given); a cell's bits
//               depend neither on R nor on the rest of the batch.
//   the DP      one workgroup per utterance sweeps the anti-diagonals: cell (t,u) of diagonal d reads its predecessors from
//               diagonal d - 1 (standard) or d - 1 and d - 2 (one per frame).  The last three diagonals of both recursions live in
//               LDS, indexed by u; one barrier per diagonal.  Every cell is one fixed expression of two predecessors, so the
//               result does not depend on how cells are spread over lanes.  Viterbi back-pointers are one bit per cell
//               (1 = the label predecessor), written per wave by ballot; thread 0 walks them back and writes frames, wave 0 then reads
//               logp off the lattice.
// THESE GPUS ARE SHARED: the plan kernel checks every count against u_cap and every id against the vocabulary (the blank is no
// label) before anything indexes with them; a bad row has no lattice cells, its outputs are NaN / -1 and the call returns
// RS_EINVAL after the sync.  Compiled with -ffp-contract=off.
//
// rs_rnnt_align_rows: R text rows, row r scored against the frames of utterance row_utt[r].  Everything above holds with "text row"
// for "utterance"; only the joint-encoder frames and enc_lens are read through row_utt.  The plan (rs_align_rows_plan.h) gives every
// row with a lattice m(r) and donor(r): the row owns the columns u >= m of its lattice, a T x (U - m + 1) lattice in the same
// anti-diagonal order (lat_off / lat_index with U - m), and its compacted list holds those cells alone.  Column m is recomputed —
// lb(t, m) is the donor's, ly(t, m) picks another label from the same logits — so the pick kernel stays as it is.  The DP of a
// row walks its donor chain once into LDS (at most 64 entries: first lattice row, U, m) and one byte per column names the
// chain entry that owns it; a predecessor's lb / ly is then read from its owner's list.  The cells read are, bit for bit, the
// cells the row would have computed: a cell's bits depend on the utterance, the frame and the label prefix only.  rs_rnnt_align
// itself runs the kernels it ran (no row_utt, no chain: the template arguments below).
#include "k_rnnt_common.h"
#include "rs_align_rows_plan.h"

namespace {

constexpr int ALIGN_U_MAX = RS_ALIGN_U_CAP_MAX;             // u_cap bound: three diagonals of U + 1 cells for two recursions fit 48 KiB of LDS
constexpr int ALIGN_CELLS = ALIGN_U_MAX + 1;
constexpr int ALIGN_THREADS = 256;

struct AlignArgs {
    const int32_t* enc_lens;   // [B]
    const int32_t* ids;        // [B][u_cap]
    const int32_t* n_ids;      // [B]
    int B, u_cap, tp_max, V, blank, one;                    // B: the text rows (rs_rnnt_align: one per utterance)
    const int32_t* row_utt;    // [B] rs_rnnt_align_rows: the utterance of text row b (nullptr: row b is utterance b)
    int n_utt, no_sharing;
    // workspace
    int32_t* n_ok;             // [B] U, or -1 for a bad row
    int32_t* t_of;             // [B] T = min(enc_lens, tp_max), at least 0
    int32_t* base;             // [B + 1] first lattice row of utterance b; base[b + 1] - base[b] = T (U + 1), or 0 without a lattice
    int32_t* info;             // [0] rows in all, [1] longest U + 1 among the utterances with a lattice, [2] a bad entry was met
    float* lat_b;              // [rows] lb of lattice row w
    float* lat_y;              // [rows] ly of lattice row w (unused at u = U)
    uint32_t* bits;            // [B][tp_max + u_cap + 1][bit_words] Viterbi back-pointers of diagonal d, bit u
    int bit_words;
    int32_t* lat_u;            // rs_rnnt_align_rows, [B] each: U of a row with a lattice else -1; m(b); donor(b) or -1
    int32_t* m_of;
    int32_t* donor;
    int32_t* row_b;            // [R] text row, frame and label index of the current chunk's rows
    int32_t* row_t;
    int32_t* row_u;
};

// cells of the T x (U + 1) lattice on the anti-diagonals before d (T >= 1, 0 <= d <= T + U)
__host__ __device__ __forceinline__ int lat_off(int T, int U, int d) {
    const int m = (T - 1 < U ? T - 1 : U), M = (T - 1 < U ? U : T - 1);
    if (d <= m + 1) return d * (d + 1) / 2;
    if (d <= M + 1) return (m + 1) * (m + 2) / 2 + (d - m - 1) * (m + 1);
    const int n = T + U - d;
    return T * (U + 1) - n * (n + 1) / 2;
}
__host__ __device__ __forceinline__ int lat_ulo(int T, int d) { return d - T + 1 > 0 ? d - T + 1 : 0; }
// lattice row of cell (t, u) within its utterance
__device__ __forceinline__ int lat_index(int T, int U, int t, int u) { return lat_off(T, U, t + u) + u - lat_ulo(T, t + u); }

// lattice row w -> (b, t, u); w < info[0]
__device__ __forceinline__ void lat_cell(const AlignArgs& a, int w, int& b, int& t, int& u) {
    int lo = 0, hi = a.B - 1;                               // the last b with base[b] <= w (empty utterances share a base: skipped)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.base[mid] <= w) lo = mid; else hi = mid - 1;
    }
    b = lo;
    const int m = a.m_of ? a.m_of[b] : 0;                   // the row owns the columns m .. U: a T x (U - m + 1) lattice
    const int i = w - a.base[b], T = a.t_of[b], U = a.n_ok[b] - m;
    int dl = 0, dh = T + U - 1;                             // the last d with lat_off(d) <= i
    while (dl < dh) {
        const int mid = (dl + dh + 1) >> 1;
        if (lat_off(T, U, mid) <= i) dl = mid; else dh = mid - 1;
    }
    u = lat_ulo(T, dl) + (i - lat_off(T, U, dl));
    t = dl - u;
    u += m;
}

// ---- the plan: counts, checks and the lattice's prefix sums.  One workgroup: thread i owns a contiguous run of utterances. ----
__global__ __launch_bounds__(256) void align_plan_kernel(AlignArgs a) {
    __shared__ int part[256];
    __shared__ int longest_s, bad_s;
    const int tid = threadIdx.x;
    if (tid == 0) { longest_s = 0; bad_s = 0; }
    __syncthreads();
    const int per = (a.B + 255) / 256;
    const int b0 = tid * per, b1 = (b0 + per) < a.B ? (b0 + per) : a.B;
    int sum = 0, longest = 0, bad = 0;
    for (int b = b0; b < b1; ++b) {
        int n = a.n_ids[b];
        if (n < 0 || n > a.u_cap) n = -1;
        for (int u = 0; u < n; ++u) {
            const int id = a.ids[(size_t)b * a.u_cap + u];
            if (id < 0 || id >= a.V || id == a.blank) { n = -1; break; }
        }
        int T = a.enc_lens[b];
        T = T < a.tp_max ? T : a.tp_max;
        T = T > 0 ? T : 0;
        a.n_ok[b] = n;
        a.t_of[b] = T;
        if (n < 0) { bad = 1; continue; }
        if (T == 0 || (a.one && n > T)) continue;           // nothing to score: the empty alignment or an infeasible text
        sum += T * (n + 1);
        longest = n + 1 > longest ? n + 1 : longest;
    }
    part[tid] = sum;
    if (longest) atomicMax(&longest_s, longest);
    if (bad) atomicOr(&bad_s, 1);
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        a.info[0] = run; a.info[1] = longest_s; a.info[2] = bad_s;
        a.base[a.B] = run;
    }
    __syncthreads();
    int w = part[tid];
    for (int b = b0; b < b1; ++b) {
        const int n = a.n_ok[b], T = a.t_of[b];
        a.base[b] = w;
        if (n >= 0 && T > 0 && !(a.one && n > T)) w += T * (n + 1);
    }
}

// ---- the plan of rs_rnnt_align_rows: row_utt is checked first (nothing indexes with it before), then the rows as above, then
// m and donor of every row with a lattice, and the prefix sums over the rows each one owns.  One workgroup, as above. ----
// info: [0] owned rows in all, [1] longest U + 1, [2] a bad text, [3] what row_utt does wrong (RS_ROWS_*), [4] rows without sharing
__global__ __launch_bounds__(256) void align_rows_plan_kernel(AlignArgs a) {
    __shared__ int part[256];
    __shared__ int longest_s, bad_s, err_s, full_s;
    const int tid = threadIdx.x;
    if (tid == 0) { longest_s = 0; bad_s = 0; err_s = 0; full_s = 0; }
    __syncthreads();
    const int per = (a.B + 255) / 256;
    const int b0 = tid * per < a.B ? tid * per : a.B, b1 = (b0 + per) < a.B ? (b0 + per) : a.B;
    int err = 0;
    for (int b = b0; b < b1; ++b) err |= rs_align_rows_check_row(a.row_utt, a.n_utt, b);
    if (err) atomicOr(&err_s, err);
    __syncthreads();
    if (err_s) {                                            // nothing is scored and nothing is written
        if (tid == 0) { a.info[0] = 0; a.info[1] = 0; a.info[2] = 0; a.info[3] = err_s; a.info[4] = 0; }
        return;
    }
    int bad = 0;
    for (int b = b0; b < b1; ++b) {
        const int utt = a.row_utt[b];
        int T = 0, n = -1, lu = RS_ROWS_NO_LATTICE;
        if (utt >= 0) {
            T = a.enc_lens[utt];
            T = T < a.tp_max ? T : a.tp_max;
            T = T > 0 ? T : 0;
            n = a.n_ids[b];
            lu = rs_align_rows_lattice_u(n, a.ids + (size_t)b * a.u_cap, a.u_cap, a.V, a.blank, T, a.one);
            if (lu == RS_ROWS_BAD) { bad = 1; n = -1; }
        }
        a.n_ok[b] = n;                                      // -1: skipped (row_utt -1) or bad
        a.t_of[b] = T;
        a.lat_u[b] = lu >= 0 ? lu : -1;
    }
    if (bad) atomicOr(&bad_s, 1);
    __syncthreads();
    int sum = 0, full = 0, longest = 0;
    for (int b = b0; b < b1; ++b) {
        int m = 0, from = -1;
        const int U = a.lat_u[b];
        if (U >= 0) {
            if (!a.no_sharing) rs_align_rows_share(a.row_utt, a.lat_u, a.ids, a.u_cap, b, &m, &from);
            sum += a.t_of[b] * (U + 1 - m);
            full += a.t_of[b] * (U + 1);
            longest = U + 1 > longest ? U + 1 : longest;
        }
        a.m_of[b] = m;
        a.donor[b] = from;
    }
    part[tid] = sum;
    if (longest) atomicMax(&longest_s, longest);
    if (full) atomicAdd(&full_s, full);
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        a.info[0] = run; a.info[1] = longest_s; a.info[2] = bad_s; a.info[3] = 0; a.info[4] = full_s;
        a.base[a.B] = run;
    }
    __syncthreads();
    int w = part[tid];
    for (int b = b0; b < b1; ++b) {
        a.base[b] = w;
        if (a.lat_u[b] >= 0) w += a.t_of[b] * (a.lat_u[b] + 1 - a.m_of[b]);
    }
}

__device__ __forceinline__ bool has_lattice(const AlignArgs& a, int b) { return a.base[b + 1] > a.base[b]; }

// ---- the chunk's rows w0 .. w0 + n -> (b, t, u), once for the kernels that follow ----
__global__ __launch_bounds__(256) void align_rows_kernel(AlignArgs a, int w0, int n) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int b, t, u;
    lat_cell(a, w0 + r, b, t, u);
    a.row_b[r] = b; a.row_t[r] = t; a.row_u[r] = u;
}

// ---- LSTM families, step u of the chain (u = 0 .. longest U): the rows with a lattice and u <= U take their previous label ----
__global__ __launch_bounds__(256) void align_lstm_step_kernel(AlignArgs a, DecodeState st, int u) {
    __shared__ int n_act_s;
    if (threadIdx.x == 0) n_act_s = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < a.B; b += 256) {
        if (!has_lattice(a, b) || u > a.n_ok[b]) continue;
        st.token[b] = u > 0 ? a.ids[(size_t)b * a.u_cap + u - 1] : a.blank;     // checked by the plan
        st.act[atomicAdd(&n_act_s, 1)] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) st.counters[0] = n_act_s;
}

// ---- Zipformer family, chunk rows w0 .. w0 + n: decoder row r takes the two tokens before label u + 1 of its utterance ----
__global__ __launch_bounds__(256) void align_k2_context_kernel(AlignArgs a, DecodeState st, int n) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) st.counters[0] = n;
    if (r >= n) return;
    const int b = a.row_b[r], u = a.row_u[r];
    const int t1 = u >= 1 ? a.ids[(size_t)b * a.u_cap + u - 1] : a.blank;
    const int t0 = u >= 2 ? a.ids[(size_t)b * a.u_cap + u - 2] : (u == 1 ? a.blank : -1);
    st.token2[r] = t0; st.token[r] = t1; st.act[r] = r;
}

// ---- a_pre[r] = act(f[b][t] + g(u)) of the chunk's rows, and the tile kernel's row list (the identity) ----
// g_log != nullptr: g(u) of utterance b is g_log[u][b][:] (LSTM families); else st.g[r][:] (this chunk's decoder launch)
__global__ __launch_bounds__(256) void align_gather_kernel(AlignArgs a, DecodeState st, const float* __restrict__ f,
                                                           const float* __restrict__ g_log, float* __restrict__ a_pre, int J,
                                                           int n, int list_pitch, int parity) {
    const int j4 = J / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * j4) return;
    const int r = (int)(i / j4), k = (int)(i - (long long)r * j4) * 4;
    const int b = a.row_b[r], t = a.row_t[r], u = a.row_u[r];
    const int fb = a.row_utt ? a.row_utt[b] : b;             // (checked by the plan)
    const float4 fv = *reinterpret_cast<const float4*>(f + ((size_t)fb * a.tp_max + t) * J + k);
    const float* gr = g_log ? g_log + ((size_t)u * a.B + b) * J : st.g + (size_t)r * J;
    const float4 gv = *reinterpret_cast<const float4*>(gr + k);
    *reinterpret_cast<float4*>(a_pre + (size_t)r * J + k) = rs_joint_act4(fv, gv, st.joint_act);
    if (k == 0) st.alive[(size_t)parity * list_pitch + r] = r;
    if (i == 0) st.counters[2 + parity] = n;
}

// ---- log-softmax pick: one wave per row of the chunk, the reduction order of rnnt_logp_pick_kernel; two numbers per cell ----
__global__ __launch_bounds__(256) void align_pick_kernel(AlignArgs a, const float* __restrict__ z, int zstride, int w0, int n) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* zr = z + (size_t)r * zstride;
    const int V = a.V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) {
        const float x = zr[v];
        if (x > m) m = x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(m, off, 64);
        if (ov > m) m = ov;
    }
    // lane-strided sums over v < V only, then the 32 -> 1 tree: after the step `off`, lanes l < off hold p[l] + p[l + off]
    float p = 0.0f;
    for (int v = lane; v < V; v += 64) p = p + rs_expf(zr[v] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p = p + __shfl_down(p, off, 64);
    if (lane == 0) {
        const int b = a.row_b[r], u = a.row_u[r];
        const float lse = m + rs_logf(p);
        a.lat_b[w0 + r] = zr[a.blank] - lse;
        if (u < a.n_ok[b]) a.lat_y[w0 + r] = zr[a.ids[(size_t)b * a.u_cap + u]] - lse;
    }
}

__device__ __forceinline__ float lae(float x, float y) {
    const float m = x >= y ? x : y;
    if (m == -INFINITY) return m;
    return m + rs_logf(rs_expf(x - m) + rs_expf(y - m));
}

// ---- the DP: one workgroup per text row.  SHARED (rs_rnnt_align_rows with sharing): the columns u < m of the row are read from
// its donor chain; otherwise every cell is the row's own and the lattice is addressed as rs_rnnt_align always did ----
template <bool SHARED>
__global__ __launch_bounds__(ALIGN_THREADS) void align_dp_kernel(AlignArgs a, float* __restrict__ loglik, float* __restrict__ best,
                                                                int32_t* __restrict__ frames, float* __restrict__ logp) {
    __shared__ float al[3][ALIGN_CELLS];      // the forward sum on diagonals d, d - 1, d - 2 (slot d % 3), indexed by u
    __shared__ float vi[3][ALIGN_CELLS];      // the Viterbi score
    __shared__ uint8_t own[SHARED ? ALIGN_CELLS : 1];                    // chain entry that owns column u
    __shared__ int ch_base[SHARED ? RS_ALIGN_ROWS_PER_UTT_MAX : 1];     // per chain entry: first lattice row, U, m
    __shared__ int ch_u[SHARED ? RS_ALIGN_ROWS_PER_UTT_MAX : 1];
    __shared__ int ch_m[SHARED ? RS_ALIGN_ROWS_PER_UTT_MAX : 1];
    __shared__ int ch_hi[SHARED ? RS_ALIGN_ROWS_PER_UTT_MAX : 1];       // the entry owns the columns ch_m .. ch_hi - 1 of this row
    __shared__ int ch_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int U = a.n_ok[b], T = a.t_of[b];
    const float nan = __uint_as_float(0x7fc00000u);
    float* lp = logp + (size_t)b * a.u_cap;
    int32_t* fr = frames + (size_t)b * a.u_cap;
    if (U < 0) {                                             // a bad row: a count outside 0..u_cap, or an id that is no label
        if (a.row_utt && a.row_utt[b] == -1) return;         // a skipped row: no slot of it is touched
        int n = a.n_ids[b];
        n = n < 0 ? 0 : (n > a.u_cap ? a.u_cap : n);
        for (int u = tid; u < n; u += ALIGN_THREADS) { fr[u] = -1; lp[u] = nan; }
        if (tid == 0) { loglik[b] = nan; best[b] = nan; }
        return;
    }
    if (!has_lattice(a, b)) {
        const bool empty = T == 0 && U == 0;                 // the empty alignment of an empty text; else infeasible
        for (int u = tid; u < U; u += ALIGN_THREADS) { fr[u] = -1; lp[u] = nan; }
        if (tid == 0) { loglik[b] = empty ? 0.0f : -INFINITY; best[b] = empty ? 0.0f : -INFINITY; }
        return;
    }
    const float* lb = a.lat_b + a.base[b];
    const float* ly = a.lat_y + a.base[b];
    const int one = a.one;
    if (SHARED) {
        if (tid == 0) {                                      // the chain: this row, its donor, the donor's donor .. (donor < row)
            int q = b, hi = U + 1, k = 0;
            for (; k < RS_ALIGN_ROWS_PER_UTT_MAX; ++k) {
                const int mq = a.m_of[q];
                ch_base[k] = a.base[q]; ch_u[k] = a.n_ok[q]; ch_m[k] = mq; ch_hi[k] = hi;
                hi = mq < hi ? mq : hi;
                q = a.donor[q];
                if (hi == 0 || q < 0) { ++k; break; }
            }
            ch_n = k;
        }
        __syncthreads();
        for (int u = tid; u <= U; u += ALIGN_THREADS) {
            int k = 0;
            while (k + 1 < ch_n && !(u >= ch_m[k] && u < ch_hi[k])) ++k;
            own[u] = (uint8_t)k;
        }
        __syncthreads();
    }
    // lattice row (in the whole list) of cell (t, u) of this row, through the owner of column u
    auto cell_row = [&](int t, int u) -> int {
        const int k = own[u], mk = ch_m[k];
        return ch_base[k] + lat_index(T, ch_u[k] - mk, t, u - mk);
    };
    const int n_diag = one ? T + U + 1 : T + U;              // diagonals d = t + u with a cell
    const int t_top = one ? T : T - 1;                       // the largest t of the DP's cells
    uint32_t* bits = a.bits + (size_t)b * (a.tp_max + a.u_cap + 1) * a.bit_words;
    for (int d = 0; d < n_diag; ++d) {
        const int ulo = d - t_top > 0 ? d - t_top : 0, uhi = d < U ? d : U;
        float* al_d = al[d % 3];
        float* vi_d = vi[d % 3];
        const float* al_1 = al[(d + 2) % 3];
        const float* vi_1 = vi[(d + 2) % 3];
        const float* al_2 = one ? al[(d + 1) % 3] : al_1;    // where the label predecessor lives
        const float* vi_2 = one ? vi[(d + 1) % 3] : vi_1;
        // lattice rows of the predecessors' diagonals: the blank term reads lb(t - 1, u) on lattice diagonal d - 1; the label term
        // reads ly(t, u - 1) on d - 1 (standard) or ly(t - 1, u - 1) on d - 2 (one per frame)
        const int dy = one ? d - 2 : d - 1;
        const int ob = d >= 1 ? lat_off(T, U, d - 1) - lat_ulo(T, d - 1) : 0;
        const int oy = dy >= 0 ? lat_off(T, U, dy) - lat_ulo(T, dy) : 0;
        for (int u0 = (ulo / ALIGN_THREADS) * ALIGN_THREADS; u0 <= uhi; u0 += ALIGN_THREADS) {       // block-uniform
            const int u = u0 + tid, t = d - u;
            const bool cell = u >= ulo && u <= uhi;
            bool from_label = false;
            if (cell) {
                float sa, va;
                if (d == 0) {
                    sa = 0.0f; va = 0.0f;
                } else {
                    float ab = -INFINITY, vb = -INFINITY, ay = -INFINITY, vy = -INFINITY;
                    if (t >= 1) {                                                    // (t - 1, u): u <= d - 1
                        const float x = SHARED ? a.lat_b[cell_row(t - 1, u)] : lb[ob + u];
                        ab = al_1[u] + x; vb = vi_1[u] + x;
                    }
                    if (u >= 1 && (!one || t >= 1)) {
                        const float x = SHARED ? a.lat_y[cell_row(one ? t - 1 : t, u - 1)] : ly[oy + u - 1];
                        ay = al_2[u - 1] + x; vy = vi_2[u - 1] + x;
                    }
                    sa = lae(ab, ay);
                    from_label = vy > vb;                                            // ties go to the blank predecessor
                    va = from_label ? vy : vb;
                }
                al_d[u] = sa; vi_d[u] = va;
            }
            const unsigned long long word = __ballot(from_label);                    // this wave's 64 cells u0 + 64 wave ..
            if ((tid & 63) == 0 && u <= uhi && u + 63 >= ulo) {
                const int w32 = (u0 + tid) >> 5;
                if (w32 < a.bit_words) bits[(size_t)d * a.bit_words + w32] = (uint32_t)word;
                if (w32 + 1 < a.bit_words) bits[(size_t)d * a.bit_words + w32 + 1] = (uint32_t)(word >> 32);
            }
        }
        __syncthreads();
    }
    // the last diagonal holds one cell, (t_top, U)
    if (tid == 0) {
        const int d = n_diag - 1;
        const float x = one ? 0.0f : (SHARED ? a.lat_b[cell_row(T - 1, U)] : lb[lat_index(T, U, T - 1, U)]);
        loglik[b] = one ? al[d % 3][U] : al[d % 3][U] + x;
        best[b] = one ? vi[d % 3][U] : vi[d % 3][U] + x;
        // walk the back-pointers from (t_top, U): at most T + U steps
        int t = t_top, u = U;
        for (int step = 0; step < T + U + 1 && u > 0; ++step) {
            const int dd = t + u;
            const bool from_label = (bits[(size_t)dd * a.bit_words + (u >> 5)] >> (u & 31)) & 1u;
            if (from_label) {
                fr[u - 1] = one ? t - 1 : t;
                --u;
                if (one) --t;
            } else {
                if (t == 0) break;                           // cannot happen: at t = 0 only the label predecessor is finite
                --t;
            }
        }
        for (; u > 0; --u) fr[u - 1] = -1;                    // (unreachable; no slot stays unwritten)
    }
    __syncthreads();
    if (tid < 64)
        for (int u = tid; u < U; u += 64) {
            const int t = fr[u];
            lp[u] = (t >= 0 && t < T) ? (SHARED ? a.lat_y[cell_row(t, u)] : ly[lat_index(T, U, t, u)]) : nan;
        }
}

// ---- workspace ----
struct AlignLayout {
    DecodeState st{};
    AlignArgs a{};
    float* g_log = nullptr;    // LSTM families: [u_cap + 1][B][J]
    float* a_pre = nullptr;    // [R][J]
};

// R = rows per chunk (a multiple of 32); B = the text rows; rows: the form of rs_rnnt_align_rows (three more arrays, at the end)
void align_layout(const rs_ctx* ctx, int B, int tp_max, int u_cap, size_t R, bool rows, rs_arena& ar, AlignLayout& l) {
    const rs_dims& d = ctx->d;
    const size_t H = d.pred_hidden, J = d.joint_hidden, cells = (size_t)B * tp_max * (u_cap + 1);
    DecodeState& st = l.st;
    l.a.bit_words = (u_cap + 1 + 63) / 64 * 2;
    l.a.n_ok = ar.take<int32_t>(B);
    l.a.t_of = ar.take<int32_t>(B);
    l.a.base = ar.take<int32_t>((size_t)B + 1);
    l.a.info = ar.take<int32_t>(16);
    l.a.lat_b = ar.take<float>(cells);
    l.a.lat_y = ar.take<float>(cells);
    l.a.bits = ar.take<uint32_t>((size_t)B * (tp_max + u_cap + 1) * l.a.bit_words);
    l.a.row_b = ar.take<int32_t>(R); l.a.row_t = ar.take<int32_t>(R); l.a.row_u = ar.take<int32_t>(R);
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
        l.g_log = ar.take<float>((size_t)B * (u_cap + 1) * J);
        st.g = l.g_log;
    }
    st.alive = ar.take<int32_t>(2 * R);                                      // [2][R]: the tile kernel reads list (chunk & 1) at pitch R
    l.a_pre = ar.take<float>(R * J);
    st.zapprox = ar.take<float>(R * (size_t)rs_joint_zstride(d));
    st.a_pre = l.a_pre;
    st.joint_act = d.joint_act;
    if (rows) { l.a.lat_u = ar.take<int32_t>(B); l.a.m_of = ar.take<int32_t>(B); l.a.donor = ar.take<int32_t>(B); }
}
constexpr size_t ALIGN_MAX_R = 32 * 65535;                 // the tile kernel's grid

size_t align_bytes(const rs_ctx* ctx, int B, int tp_max, int u_cap, size_t R, bool rows) {
    rs_arena ar;
    AlignLayout l;
    align_layout(ctx, B, tp_max, u_cap, R, rows, ar, l);
    return ar.bytes() + RS_DECODE_SLACK;
}

bool align_dims_ok(int B, int tp_max, int u_cap) {
    return u_cap <= ALIGN_U_MAX && (long long)B * tp_max * (u_cap + 1) <= 0x3fffffffLL && (long long)B * (u_cap + 1) <= 0x3fffffffLL;
}


// rows per chunk that `workspace_bytes` holds (0: below the minimum), at most the rows there can be
size_t align_chunk_rows(const rs_ctx* ctx, int B, int tp_max, int u_cap, bool rows, size_t workspace_bytes) {
    const size_t least = align_bytes(ctx, B, tp_max, u_cap, 32, rows);
    if (workspace_bytes < least) return 0;
    const size_t per32 = align_bytes(ctx, B, tp_max, u_cap, 64, rows) - least;
    size_t most = ((size_t)B * tp_max * (u_cap + 1) + 31) / 32 * 32;
    if (most < 32) most = 32;
    if (most > ALIGN_MAX_R) most = ALIGN_MAX_R;
    size_t R = 32 + 32 * ((workspace_bytes - least) / per32);
    if (R > most) R = most;
    while (R > 32 && align_bytes(ctx, B, tp_max, u_cap, R, rows) > workspace_bytes) R -= 32;
    return R;
}

// B text rows; row_utt == nullptr: rs_rnnt_align (row b is utterance b, n_utt = B), else rs_rnnt_align_rows over n_utt utterances
int align_run(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int n_utt, int tp_max, const int32_t* row_utt, int B,
              const int32_t* ids, const int32_t* n_ids, int u_cap, int one_per_frame, int no_sharing, float* loglik, float* best,
              int32_t* frames, float* logp, int64_t* stats, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const rs_dims& d = ctx->d;
    const int L = d.pred_layers, H = d.pred_hidden, J = d.joint_hidden, V = d.n_logits;
    const bool k2 = ctx->k2_conv_w != nullptr, rows = row_utt != nullptr;
    if (int rc = rs_rnnt_check_dims(ctx, "align"); rc != RS_OK) return rc;
    if (k2 && L != 1) return rs_fail(ctx, RS_EINVAL, "align: unsupported prediction network");
    if (!align_dims_ok(B, tp_max, u_cap)) return rs_fail(ctx, RS_EINVAL, "align: u_cap above %d or B x tp_max x (u_cap + 1) too large", ALIGN_U_MAX);
    const size_t R = align_chunk_rows(ctx, B, tp_max, u_cap, rows, workspace_bytes);
    if (R == 0)
        return rs_fail(ctx, RS_EINVAL, "align: workspace %zu < %zu", workspace_bytes, align_bytes(ctx, B, tp_max, u_cap, 32, rows));
    rs_arena arena(workspace);
    AlignLayout l;
    align_layout(ctx, B, tp_max, u_cap, R, rows, arena, l);
    DecodeState& st = l.st;
    AlignArgs& a = l.a;
    a.enc_lens = enc_lens; a.ids = ids; a.n_ids = n_ids;
    a.B = B; a.u_cap = u_cap; a.tp_max = tp_max; a.V = V; a.blank = d.blank_id; a.one = one_per_frame;
    a.row_utt = row_utt; a.n_utt = n_utt; a.no_sharing = no_sharing;
    if (k2) st.unk = rs_k2_unk_id(ctx);
    const int zstride = rs_joint_zstride(d);
    if (stats) stats[0] = stats[1] = 0;

    // three brackets of the decode class, in this order: the plan and the prediction chain, the lattice (its flops: the joint's
    // products over the rows), the DP
    int32_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
        if (rows) hipLaunchKernelGGL(align_rows_plan_kernel, dim3(1), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(align_plan_kernel, dim3(1), dim3(256), 0, s, a);
        RS_HIP(ctx, hipMemcpyAsync(info, a.info, rows ? sizeof info : 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RS_HIP(ctx, hipStreamSynchronize(s));
    }
    if (rows && info[3])
        return rs_fail(ctx, RS_EINVAL, "align: row_utt %s (nothing was scored)",
                       (info[3] & RS_ROWS_BAD_UTT) ? "names an utterance outside 0..B-1 (-1 skips a row)"
                       : (info[3] & RS_ROWS_DECREASE) ? "decreases" : "gives one utterance more rows than RS_ALIGN_ROWS_PER_UTT_MAX");
    const int n_rows = info[0], longest = info[1];
    if (n_rows < 0 || (long long)n_rows > (long long)B * tp_max * (u_cap + 1) || longest < 0 || longest > u_cap + 1)
        return rs_fail(ctx, RS_ESTATE, "align: inconsistent plan");
    if (stats) { stats[0] = n_rows; stats[1] = rows ? info[4] : n_rows; }
    if (!k2 && n_rows > 0) {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
        const size_t state_bytes = (size_t)L * B * H * 4;
        RS_HIP(ctx, hipMemsetAsync(st.h, 0, 2 * rs_align(state_bytes), s));
        for (int u = 0; u < longest; ++u) {
            DecodeState su = st;
            su.g = l.g_log + (size_t)u * B * J;           // the projection writes row b of step u's slab
            hipLaunchKernelGGL(align_lstm_step_kernel, dim3(1), dim3(256), 0, s, a, su, u);
            if (int rc = rs_rnnt_launch_lstm_pred(ctx, &su, B, s); rc != RS_OK) return rc;
        }
    }
    if (n_rows > 0) {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 2.0 * n_rows * (double)J * V, 4.0 * n_rows * ((double)J + zstride));
        int chunk = 0;
        for (int w0 = 0; w0 < n_rows; w0 += (int)R, ++chunk) {
            const int n = n_rows - w0 < (int)R ? n_rows - w0 : (int)R;
            hipLaunchKernelGGL(align_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, w0, n);
            if (k2) {
                hipLaunchKernelGGL(align_k2_context_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, st, n);
                if (int rc = rs_rnnt_launch_lstm_pred(ctx, &st, n, s); rc != RS_OK) return rc;
            }
            const long long n_thr = (long long)n * (J / 4);
            hipLaunchKernelGGL(align_gather_kernel, dim3((unsigned)((n_thr + 255) / 256)), dim3(256), 0, s, a, st, joint_enc,
                               (const float*)(k2 ? nullptr : l.g_log), l.a_pre, J, n, (int)R, chunk & 1);
            if (int rc = rs_rnnt_launch_joint_logits_indirect(ctx, &st, joint_enc, (int)R, n, tp_max, 1, chunk, s); rc != RS_OK) return rc;
            hipLaunchKernelGGL(align_pick_kernel, dim3((n + 3) / 4), dim3(256), 0, s, a, st.zapprox, zstride, w0, n);
        }
        RS_CHECK_LAUNCH(ctx, "align: lattice");
    }
    {
        rs_prof_scope prof(ctx, RS_PROF_DECODE, s, 0.0, 0.0);
        if (rows && !no_sharing)
            hipLaunchKernelGGL(align_dp_kernel<true>, dim3(B), dim3(ALIGN_THREADS), 0, s, a, loglik, best, frames, logp);
        else
            hipLaunchKernelGGL(align_dp_kernel<false>, dim3(B), dim3(ALIGN_THREADS), 0, s, a, loglik, best, frames, logp);
        RS_CHECK_LAUNCH(ctx, "align: dp");
        RS_HIP(ctx, hipStreamSynchronize(s));
    }
    if (info[2]) return rs_fail(ctx, RS_EINVAL, "align: a count outside 0..u_cap, or an id outside the vocabulary or the blank in a text (its row is NaN / -1)");
    return RS_OK;
}

}  // namespace

size_t rs_rnnt_align_workspace_bytes_impl(const rs_ctx* ctx, int B, int tp_max, int u_cap) {
    return align_dims_ok(B, tp_max, u_cap) ? align_bytes(ctx, B, tp_max, u_cap, 32, false) : 0;
}

size_t rs_rnnt_align_rows_workspace_bytes_impl(const rs_ctx* ctx, int R, int tp_max, int u_cap) {
    return align_dims_ok(R, tp_max, u_cap) ? align_bytes(ctx, R, tp_max, u_cap, 32, true) : 0;
}

int rs_rnnt_align_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* ids,
                       const int32_t* n_ids, int u_cap, int one_per_frame, float* loglik, float* best, int32_t* frames, float* logp,
                       void* workspace, size_t workspace_bytes, hipStream_t s) {
    return align_run(ctx, joint_enc, enc_lens, B, tp_max, nullptr, B, ids, n_ids, u_cap, one_per_frame, 0, loglik, best, frames, logp,
                     nullptr, workspace, workspace_bytes, s);
}

int rs_rnnt_align_rows_impl(rs_ctx* ctx, const float* joint_enc, const int32_t* enc_lens, int B, int tp_max, const int32_t* row_utt,
                            int R, const int32_t* ids, const int32_t* n_ids, int u_cap, int one_per_frame, int no_sharing,
                            float* loglik, float* best, int32_t* frames, float* logp, int64_t* stats, void* workspace,
                            size_t workspace_bytes, hipStream_t s) {
    return align_run(ctx, joint_enc, enc_lens, B, tp_max, row_utt, R, ids, n_ids, u_cap, one_per_frame, no_sharing, loglik, best,
                     frames, logp, stats, workspace, workspace_bytes, s);
}
