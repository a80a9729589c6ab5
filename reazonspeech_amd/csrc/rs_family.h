// rs_family.h — which model family a context belongs to, and which entry points serve it (host only, plain C++: no HIP include).
//
// One rs_ctx serves three families that are not built alike: Conformer (rs_create: NeMo and ESPnet, told apart by rs_dims switches),
// Zipformer (rs_k2_create) and AV-HuBERT (rs_avsr_create).  The create function sets the tag once; RS_ENTRIES below has one row for
// every function of include/rs_asr.h whose first parameter is the context, and every such function starts with the guard
// (rs_common.h: RS_GUARD / RS_GUARD_QUERY), which refuses in this order:
//   1. a null context                      RS_EINVAL
//   2. a family the entry does not serve   RS_EINVAL  "<entry>: not defined for <a family> context" plus the row's hint
//   3. a context that is not finalized     RS_ESTATE  "rs_finalize must precede <entry>"           (rows marked FINAL only)
// The family comes before the finalized test, so a wrong pairing is refused without any weights.  Queries that return a size or a
// frame count answer 0 on a failed guard and leave the context's error text alone (their context is const; 0 is their convention).
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "../../include/rs_asr.h"

enum rs_family { RS_FAM_CONFORMER, RS_FAM_ZIPFORMER, RS_FAM_AVSR };
enum { RS_SERVES_C = 1 << RS_FAM_CONFORMER, RS_SERVES_Z = 1 << RS_FAM_ZIPFORMER, RS_SERVES_A = 1 << RS_FAM_AVSR,
       RS_SERVES_CZ = RS_SERVES_C | RS_SERVES_Z, RS_SERVES_ALL = RS_SERVES_CZ | RS_SERVES_A };
enum { RS_ANYTIME = 0, RS_FINAL = 1 };

#define RS_HINT_AVSR_ONLY "the rs_avsr_* entries take a context made by rs_avsr_create"
#define RS_HINT_LSTM_ONLY "a Zipformer context has a stateless decoder; only rs_rnnt_greedy applies (sherpa-onnx greedy_search)"
#define RS_HINT_MBS "modified beam search is defined for a Zipformer context (stateless decoder) only; a context with an LSTM prediction network takes rs_rnnt_alsd / rs_rnnt_beam"
#define RS_HINT_TRANSDUCER "defined for the transducer families; an AV-HuBERT context has no joint network and takes the rs_avsr_* entries"
#define RS_HINT_DIMS "the operator reads the Conformer dimensions (rs_dims)"

// X(entry, families served, RS_FINAL / RS_ANYTIME, hint)
#define RS_ENTRIES(X)                                                                                                                 \
    X(rs_destroy, ALL, ANYTIME, "")                                                                                                   \
    X(rs_last_error, ALL, ANYTIME, "")                                                                                                \
    X(rs_set_tensor, ALL, ANYTIME, "")                                                                                                \
    X(rs_finalize, ALL, ANYTIME, "")                                                                                                  \
    X(rs_set_option, ALL, ANYTIME, "")                                                                                                \
    X(rs_workspace_bytes, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                            \
    X(rs_mel_frames, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                                 \
    X(rs_enc_frames, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                                 \
    X(rs_frontend_logmel, CZ, FINAL, RS_HINT_TRANSDUCER)                                                                              \
    X(rs_encoder_forward, CZ, FINAL, "an AV-HuBERT context takes rs_avsr_encoder_forward")                                            \
    X(rs_encoder_set_taps, C, ANYTIME, "a Zipformer context takes rs_k2_encoder_set_taps, an AV-HuBERT context rs_avsr_encoder_set_taps") \
    X(rs_encoder_set_ctc_out, C, ANYTIME, "only a Conformer context can have a CTC head (rs_dims.ctc_vocab)")                         \
    X(rs_k2_encoder_set_taps, Z, ANYTIME, "a Conformer context takes rs_encoder_set_taps, an AV-HuBERT context rs_avsr_encoder_set_taps") \
    X(rs_rnnt_greedy, CZ, FINAL, RS_HINT_TRANSDUCER)                                                                                  \
    X(rs_rnnt_alsd_workspace_bytes, C, ANYTIME, RS_HINT_LSTM_ONLY)                                                                    \
    X(rs_rnnt_alsd, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                      \
    /* FINAL also for the size: with all-zero arguments (tests/test_gpu_family_guards.py) a query of an ANYTIME row must answer > 0 */ \
    X(rs_rnnt_alsd_hotwords_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)                                                             \
    X(rs_rnnt_alsd_hotwords, C, FINAL, RS_HINT_LSTM_ONLY)                                                                             \
    X(rs_rnnt_alsd_lm_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)                                                                   \
    X(rs_rnnt_alsd_lm, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                   \
    X(rs_rnnt_alsd_nbest_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)                                                                \
    X(rs_rnnt_alsd_nbest, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                \
    X(rs_rnnt_beam_workspace_bytes, C, ANYTIME, RS_HINT_LSTM_ONLY)                                                                    \
    X(rs_rnnt_beam, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                      \
    X(rs_rnnt_beam_nbest_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)                                                                \
    X(rs_rnnt_beam_nbest, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                \
    X(rs_rnnt_beam_lm_workspace_bytes, C, FINAL, RS_HINT_LSTM_ONLY)                                                                   \
    X(rs_rnnt_beam_lm, C, FINAL, RS_HINT_LSTM_ONLY)                                                                                   \
    X(rs_rnnt_mbs_workspace_bytes, Z, ANYTIME, RS_HINT_MBS)                                                                           \
    X(rs_rnnt_mbs, Z, FINAL, RS_HINT_MBS)                                                                                             \
    X(rs_rnnt_mbs_hotwords_workspace_bytes, Z, ANYTIME, RS_HINT_MBS)                                                                  \
    X(rs_rnnt_mbs_hotwords, Z, FINAL, RS_HINT_MBS)                                                                                    \
    /* FINAL also for the size, as rs_rnnt_alsd_hotwords_workspace_bytes above */                                                     \
    X(rs_rnnt_mbs_lm_workspace_bytes, Z, FINAL, RS_HINT_MBS)                                                                          \
    X(rs_rnnt_mbs_lm, Z, FINAL, RS_HINT_MBS)                                                                                          \
    X(rs_rnnt_mbs_nbest_workspace_bytes, Z, FINAL, RS_HINT_MBS)                                                                       \
    X(rs_rnnt_mbs_nbest, Z, FINAL, RS_HINT_MBS)                                                                                       \
    X(rs_rnnt_token_scores_workspace_bytes, CZ, FINAL, RS_HINT_TRANSDUCER)                                                            \
    /* ANYTIME: tests/test_gpu_token_scores.py pins RS_EINVAL for a context that is not finalized; the entry tests that itself */     \
    X(rs_rnnt_token_scores, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                          \
    X(rs_rnnt_align_workspace_bytes, CZ, FINAL, RS_HINT_TRANSDUCER)                                                                   \
    /* ANYTIME, as rs_rnnt_token_scores: RS_EINVAL for a context that is not finalized; the entry tests that itself */               \
    X(rs_rnnt_align, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                                 \
    X(rs_rnnt_align_rows_workspace_bytes, CZ, FINAL, RS_HINT_TRANSDUCER)                                                              \
    X(rs_rnnt_align_rows, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                            \
    X(rs_rnnt_token_scores_rows_workspace_bytes, CZ, FINAL, RS_HINT_TRANSDUCER)                                                       \
    X(rs_rnnt_token_scores_rows, CZ, ANYTIME, RS_HINT_TRANSDUCER)                                                                     \
    X(rs_ctc_align_workspace_bytes, ALL, ANYTIME, "")                                                                                 \
    X(rs_ctc_align, ALL, ANYTIME, "")                                                                                                 \
    X(rs_ctc_find_blank, C, ANYTIME, "defined for a context with a CTC head (the ESPnet family) only")                                \
    X(rs_resample, ALL, ANYTIME, "")                                                                                                  \
    X(rs_profile_enable, ALL, ANYTIME, "")                                                                                            \
    X(rs_profile_read, ALL, ANYTIME, "")                                                                                              \
    X(rs_profile_reset, ALL, ANYTIME, "")                                                                                             \
    X(rs_profile_read_launches, ALL, ANYTIME, "")                                                                                     \
    X(rs_gemm_bf16, ALL, ANYTIME, "")                                                                                                 \
    X(rs_gemm_f32, ALL, ANYTIME, "")                                                                                                  \
    X(rs_gemm_i8q, ALL, ANYTIME, "")                                                                                                  \
    X(rs_layernorm, ALL, ANYTIME, "")                                                                                                 \
    X(rs_glu_dwconv_silu, ALL, ANYTIME, "")                                                                                           \
    X(rs_glu_dwconv_silu_layout, ALL, ANYTIME, "")                                                                                    \
    X(rs_glu_dwconv_silu_f32, ALL, ANYTIME, "")                                                                                       \
    X(rs_relpos_attention, C, ANYTIME, RS_HINT_DIMS)                                                                                  \
    X(rs_relpos_attention_f32, C, ANYTIME, RS_HINT_DIMS)                                                                              \
    X(rs_avsr_workspace_bytes, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                         \
    X(rs_avsr_encoder_forward, A, FINAL, RS_HINT_AVSR_ONLY)                                                                           \
    X(rs_avsr_encoder_set_taps, A, ANYTIME, "a Conformer context takes rs_encoder_set_taps, a Zipformer context rs_k2_encoder_set_taps") \
    X(rs_avsr_decoder_state_bytes, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                     \
    X(rs_avsr_decoder_begin, A, FINAL, RS_HINT_AVSR_ONLY)                                                                             \
    X(rs_avsr_decoder_step, A, FINAL, RS_HINT_AVSR_ONLY)                                                                              \
    X(rs_avsr_search_state_bytes, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                      \
    X(rs_avsr_search_state_bytes_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                 \
    X(rs_avsr_search_state_bytes_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                               \
    X(rs_avsr_search_begin, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                            \
    X(rs_avsr_search_begin_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                       \
    X(rs_avsr_search_begin_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                     \
    X(rs_avsr_search_step, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                             \
    X(rs_avsr_search_step_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                        \
    X(rs_avsr_search_step_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                      \
    X(rs_avsr_search_rows, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                             \
    X(rs_avsr_search_peek, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                             \
    X(rs_avsr_search_peek_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                        \
    X(rs_avsr_search_peek_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                      \
    X(rs_avsr_search_finish, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                           \
    X(rs_avsr_search_finish_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                      \
    X(rs_avsr_search_finish_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                    \
    X(rs_avsr_generate_state_bytes, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                                    \
    X(rs_avsr_generate_state_bytes_opts, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                               \
    X(rs_avsr_generate_state_bytes_scored, A, ANYTIME, RS_HINT_AVSR_ONLY)                                                             \
    X(rs_avsr_generate, A, FINAL, RS_HINT_AVSR_ONLY)                                                                                  \
    X(rs_avsr_generate_opts, A, FINAL, RS_HINT_AVSR_ONLY)                                                                             \
    X(rs_avsr_generate_scored, A, FINAL, RS_HINT_AVSR_ONLY)

enum rs_entry {
#define RS_ENTRY_ENUM(name, serves, when, hint) RS_ENTRY_##name,
    RS_ENTRIES(RS_ENTRY_ENUM)
#undef RS_ENTRY_ENUM
    RS_ENTRY_COUNT
};
struct rs_entry_row { const char* name; int serves; int needs_final; const char* hint; };
static const rs_entry_row rs_entry_rows[RS_ENTRY_COUNT] = {
#define RS_ENTRY_ROW(name, serves, when, hint) {#name, RS_SERVES_##serves, RS_##when, hint},
    RS_ENTRIES(RS_ENTRY_ROW)
#undef RS_ENTRY_ROW
};

// the family with its article, as the refusal texts name it
inline const char* rs_family_name(rs_family f) {
    return f == RS_FAM_ZIPFORMER ? "a Zipformer" : f == RS_FAM_AVSR ? "an AV-HuBERT" : "a Conformer";
}

// The guard's decision for entry `e` on a context that exists (or not), of family `fam`, finalized (or not): RS_OK, or the code with
// the text in msg (when msg is given; a query passes none).
inline int rs_family_guard(rs_entry e, bool have_ctx, rs_family fam, bool finalized, char* msg, size_t msg_bytes) {
    const rs_entry_row& row = rs_entry_rows[e];
    if (!have_ctx) {
        if (msg && msg_bytes) snprintf(msg, msg_bytes, "%s: null context", row.name);
        return RS_EINVAL;
    }
    if (!(row.serves & (1 << fam))) {
        if (msg && msg_bytes) snprintf(msg, msg_bytes, "%s: not defined for %s context%s%s", row.name, rs_family_name(fam), row.hint[0] ? "; " : "", row.hint);
        return RS_EINVAL;
    }
    if (row.needs_final && !finalized) {
        if (msg && msg_bytes) snprintf(msg, msg_bytes, "rs_finalize must precede %s", row.name);
        return RS_ESTATE;
    }
    return RS_OK;
}
