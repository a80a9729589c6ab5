/*
 * token_scores_checker.c — rs_rnnt_token_scores (reazonspeech_amd/csrc/k_rnnt_scores.hip) restated on the oracle library's
 * routines, in the device's float32 order.  TEST INFRASTRUCTURE: built by tests/token_scores_ref.py with the flags of
 * oracle/build.py and linked against the oracle library.
 *
 * For token u of utterance b (id = ids[b][u], frame t = frames[b][u], or frames[b][u] - u when they are alignment steps):
 *   g      the prediction network after the start context and the labels ids[b][0 .. u):
 *            LSTM families   rs_oracle_lstm_step per layer from the zero state over [blank, ids[b][0], .., ids[b][u - 1]], then
 *                            g[j] = rs_oracle_dot(h_top, Wp[j]) + bp[j]          (as rs_oracle_rnnt_greedy)
 *            Zipformer       rs_oracle_k2_decoder over the two tokens before u ([-1, blank] at u = 0), the same projection
 *   z      rs_oracle_joint_argmax(f[b][t], g, .., logits_out)  -> top1 = its return value (lowest index on ties)
 *   logp   z[id] - rs_oracle_lse(z, V)
 * The joint activation is the oracle library's setting (rs_oracle_set_joint_act), set by the caller.
 * A frame outside [0, min(enc_lens[b], Tp)) or an id outside [0, V): logp = NaN, top1 = -1, and the return value is -1;
 * n_ids[b] outside [0, u_cap] is clamped and returns -1 too.  Slots at u >= n_ids[b] are not written.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void rs_oracle_lstm_step(const float* x, const float* h, const float* c, const float* W, const float* bias, int H, float* h_out,
                         float* c_out);
int rs_oracle_joint_argmax(const float* f, const float* g, const float* Wo, const float* bo, int J, int V, float* logits_out);
float rs_oracle_dot(const float* a, const float* w, int K);
float rs_oracle_lse(const float* z, int V);
void rs_oracle_k2_decoder(const float* embed, const float* conv_w, int D, int t0, int t1, float* h);

int rs_token_scores_checker(const float* f, const int32_t* enc_lens, int B, int Tp, int J, int H, int L, int V, int blank,
                            const float* embed, const float* const* lstm_w, const float* const* lstm_b,
                            const float* conv_w /* non-NULL: the stateless decoder (L is ignored) */, const float* Wp,
                            const float* bp, const float* Wo, const float* bo, const int32_t* ids, const int32_t* frames,
                            const int32_t* n_ids, int u_cap, int frames_are_steps, float* logp, int32_t* top1) {
    int bad = 0;
    const int layers = conv_w ? 1 : L;
    float* h = (float*)malloc(sizeof(float) * layers * H * 2);
    float* c = (float*)malloc(sizeof(float) * layers * H * 2);
    float* g = (float*)malloc(sizeof(float) * J);
    float* z = (float*)malloc(sizeof(float) * V);
    for (int b = 0; b < B; ++b) {
        int n = n_ids[b];
        if (n < 0 || n > u_cap) { bad = 1; n = n < 0 ? 0 : u_cap; }
        float *hc = h, *hn = h + layers * H, *cc = c, *cn = c + layers * H;
        memset(h, 0, sizeof(float) * layers * H * 2);
        memset(c, 0, sizeof(float) * layers * H * 2);
        int t0 = -1, t1 = blank;                           /* the last two tokens; t1 is the LSTM's input */
        int T = enc_lens[b];
        if (T > Tp) T = Tp;
        for (int u = 0; u < n; ++u) {
            if (conv_w) {
                rs_oracle_k2_decoder(embed, conv_w, H, t0, t1, hn);
            } else {
                const float* x = embed + (size_t)t1 * H;
                for (int l = 0; l < layers; ++l) {
                    rs_oracle_lstm_step(x, hc + l * H, cc + l * H, lstm_w[l], lstm_b[l], H, hn + l * H, cn + l * H);
                    x = hn + l * H;
                }
            }
            for (int j = 0; j < J; ++j) g[j] = rs_oracle_dot(hn + (layers - 1) * H, Wp + (size_t)j * H, H) + bp[j];
            float* tmp = hc; hc = hn; hn = tmp;
            tmp = cc; cc = cn; cn = tmp;
            const size_t slot = (size_t)b * u_cap + u;
            const int id = ids[slot];
            const int t = frames[slot] - (frames_are_steps ? u : 0);
            const int id_ok = id >= 0 && id < V;
            if (!id_ok || t < 0 || t >= T) {
                bad = 1;
                logp[slot] = NAN;
                if (top1) top1[slot] = -1;
            } else {
                const int best = rs_oracle_joint_argmax(f + ((size_t)b * Tp + t) * J, g, Wo, bo, J, V, z);
                const float lse = rs_oracle_lse(z, V);
                logp[slot] = z[id] - lse;
                if (top1) top1[slot] = best;
            }
            t0 = t1;
            t1 = id_ok ? id : blank;
        }
    }
    free(h); free(c); free(g); free(z);
    return bad ? -1 : 0;
}
