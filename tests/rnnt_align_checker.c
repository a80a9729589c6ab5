/*
 * rnnt_align_checker.c — rs_rnnt_align (reazonspeech_amd/csrc/k_rnnt_align.hip) restated serially on the oracle library's
 * routines, in the device's float32 order.  TEST INFRASTRUCTURE: built by tests/rnnt_align_ref.py (checker_lib.load) with the
 * flags of oracle/build.py and linked against the oracle library.
 *
 * For utterance b with T = min(enc_lens[b], Tp) frames and the labels y_1..y_U = ids[b][0 .. U):
 *   g(u)   u = 0..U: the prediction network after the start context and the first u labels, as tests/token_scores_checker.c
 *          (rs_oracle_lstm_step per layer from the zero state / rs_oracle_k2_decoder over the last two tokens, then the projection)
 *   z      rs_oracle_joint_argmax(f[b][t], g(u), .., logits_out);  lse = rs_oracle_lse(z, V)
 *   lb(t,u) = z[blank] - lse,  ly(t,u) = z[y_(u+1)] - lse
 *   standard       a(0,0) = 0, a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t,u-1) + ly(t,u-1)),       loglik = a(T-1,U) + lb(T-1,U)
 *   one per frame  a(t,u) = lae(a(t-1,u) + lb(t-1,u), a(t-1,u-1) + ly(t-1,u-1)), t = 0..T,   loglik = a(T,U)
 *   lae(a, b)      m = max(a, b); -inf when m is -inf, else m + rs_logf(rs_expf(a - m) + rs_expf(b - m)); a is the blank term
 *   best           the recursion with max, ties to the blank predecessor; frames / logp from its path
 * The optional `lattice` receives [B][Tp][u_cap + 1][2] = (lb, ly) of every scored cell (the tests sum it along a path).
 * Bad rows (a count outside 0..u_cap, an id outside [0, V) or the blank): NaN / -1 and the return value is -1.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "rnnt_math.h"

void rs_oracle_lstm_step(const float* x, const float* h, const float* c, const float* W, const float* bias, int H, float* h_out,
                         float* c_out);
int rs_oracle_joint_argmax(const float* f, const float* g, const float* Wo, const float* bo, int J, int V, float* logits_out);
float rs_oracle_dot(const float* a, const float* w, int K);
float rs_oracle_lse(const float* z, int V);
void rs_oracle_k2_decoder(const float* embed, const float* conv_w, int D, int t0, int t1, float* h);

static float lae(float a, float b) {
    const float m = a >= b ? a : b;
    if (m == -INFINITY) return m;
    return m + rs_logf(rs_expf(a - m) + rs_expf(b - m));
}

int rs_rnnt_align_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int H, int L, int V, int blank,
                          const float* embed, const float* const* lstm_w, const float* const* lstm_b,
                          const float* conv_w /* non-NULL: the stateless decoder (L is ignored) */, const float* Wp, const float* bp,
                          const float* Wo, const float* bo, const int32_t* ids, const int32_t* n_ids, int u_cap, int one_per_frame,
                          float* loglik, float* best, int32_t* frames, float* logp, float* lattice) {
    int bad = 0;
    const int layers = conv_w ? 1 : L;
    float* h = (float*)malloc(sizeof(float) * layers * H * 2);
    float* c = (float*)malloc(sizeof(float) * layers * H * 2);
    float* g = (float*)malloc(sizeof(float) * J * (u_cap + 1));
    float* z = (float*)malloc(sizeof(float) * V);
    const size_t cells = (size_t)(Tp + 1) * (u_cap + 1);
    float* lb = (float*)malloc(sizeof(float) * cells);
    float* ly = (float*)malloc(sizeof(float) * cells);
    float* al = (float*)malloc(sizeof(float) * cells);
    float* vi = (float*)malloc(sizeof(float) * cells);
    unsigned char* bp_lab = (unsigned char*)malloc(cells);
    for (int b = 0; b < B; ++b) {
        const int32_t* y = ids + (size_t)b * u_cap;
        int32_t* fr = frames + (size_t)b * u_cap;
        float* lp = logp + (size_t)b * u_cap;
        int U = n_ids[b];
        int T = enc_lens[b];
        if (T > Tp) T = Tp;
        if (T < 0) T = 0;
        int ok = U >= 0 && U <= u_cap;
        for (int u = 0; ok && u < U; ++u) ok = y[u] >= 0 && y[u] < V && y[u] != blank;
        if (!ok) {
            bad = 1;
            const int n = U < 0 ? 0 : (U > u_cap ? u_cap : U);
            for (int u = 0; u < n; ++u) { fr[u] = -1; lp[u] = NAN; }
            loglik[b] = best[b] = NAN;
            continue;
        }
        if (T == 0 || (one_per_frame && U > T)) {
            const int empty = T == 0 && U == 0;
            for (int u = 0; u < U; ++u) { fr[u] = -1; lp[u] = NAN; }
            loglik[b] = best[b] = empty ? 0.0f : -INFINITY;
            continue;
        }
        /* g(u), u = 0..U */
        float *hc = h, *hn = h + layers * H, *cc = c, *cn = c + layers * H;
        memset(h, 0, sizeof(float) * layers * H * 2);
        memset(c, 0, sizeof(float) * layers * H * 2);
        int t0 = -1, t1 = blank;
        for (int u = 0; u <= U; ++u) {
            if (conv_w) {
                rs_oracle_k2_decoder(embed, conv_w, H, t0, t1, hn);
            } else {
                const float* x = embed + (size_t)t1 * H;
                for (int l = 0; l < layers; ++l) {
                    rs_oracle_lstm_step(x, hc + l * H, cc + l * H, lstm_w[l], lstm_b[l], H, hn + l * H, cn + l * H);
                    x = hn + l * H;
                }
            }
            for (int j = 0; j < J; ++j) g[(size_t)u * J + j] = rs_oracle_dot(hn + (layers - 1) * H, Wp + (size_t)j * H, H) + bp[j];
            float* tmp = hc; hc = hn; hn = tmp;
            tmp = cc; cc = cn; cn = tmp;
            if (u < U) { t0 = t1; t1 = y[u]; }
        }
        /* the lattice */
        const int W = u_cap + 1;
        for (int t = 0; t < T; ++t)
            for (int u = 0; u <= U; ++u) {
                rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, g + (size_t)u * J, Wo, bo, J, V, z);
                const float lse = rs_oracle_lse(z, V);
                lb[t * W + u] = z[blank] - lse;
                ly[t * W + u] = u < U ? z[y[u]] - lse : NAN;
                if (lattice) {
                    float* o = lattice + (((size_t)b * Tp + t) * W + u) * 2;
                    o[0] = lb[t * W + u]; o[1] = ly[t * W + u];
                }
            }
        /* the two recursions */
        const int t_top = one_per_frame ? T : T - 1;
        for (int t = 0; t <= t_top; ++t)
            for (int u = 0; u <= U; ++u) {
                const int i = t * W + u;
                if (t == 0 && u == 0) { al[i] = vi[i] = 0.0f; bp_lab[i] = 0; continue; }
                float ab = -INFINITY, vb = -INFINITY, ay = -INFINITY, vy = -INFINITY;
                if (t >= 1) { const float x = lb[(t - 1) * W + u]; ab = al[i - W] + x; vb = vi[i - W] + x; }
                if (one_per_frame) {
                    if (u >= 1 && t >= 1) { const float x = ly[(t - 1) * W + u - 1]; ay = al[i - W - 1] + x; vy = vi[i - W - 1] + x; }
                } else if (u >= 1) {
                    const float x = ly[t * W + u - 1]; ay = al[i - 1] + x; vy = vi[i - 1] + x;
                }
                al[i] = lae(ab, ay);
                bp_lab[i] = vy > vb;
                vi[i] = bp_lab[i] ? vy : vb;
            }
        const int last = t_top * W + U;
        if (one_per_frame) { loglik[b] = al[last]; best[b] = vi[last]; }
        else { loglik[b] = al[last] + lb[last]; best[b] = vi[last] + lb[last]; }
        int t = t_top, u = U;
        while (u > 0) {
            if (bp_lab[t * W + u]) {
                fr[u - 1] = one_per_frame ? t - 1 : t;
                --u;
                if (one_per_frame) --t;
            } else {
                --t;
            }
        }
        for (u = 0; u < U; ++u) lp[u] = ly[fr[u] * W + u];
    }
    free(h); free(c); free(g); free(z); free(lb); free(ly); free(al); free(vi); free(bp_lab);
    return bad ? -1 : 0;
}
