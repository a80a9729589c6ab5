// rs_align_rows_plan.h — the integer plan of rs_rnnt_align_rows (include/rs_asr.h): which rows may be scored, and which lattice
// columns a row of a group reads from an earlier row of its utterance.  Pure integers, plain C++, no HIP include: the plan kernel of
// k_rnnt_align.hip calls these functions on the device, tests/align_rows_host_main.cpp builds them alone on the host (also under
// AddressSanitizer + UBSan), and tests/rnnt_align_rows_ref.py restates them in numpy.
//   row_utt i32[R]   utterance of row r; -1 = the row is skipped.  The non-negative entries are non-decreasing, below B, and at most
//                    RS_ALIGN_ROWS_PER_UTT_MAX rows name one utterance.
//   lat_u i32[R]     U of a row that has a lattice (not skipped, not bad, T > 0, U <= T with one label per frame), else negative
//   m(r), donor(r)   over the earlier rows r' < r of r's utterance that have a lattice: m = the greatest number of leading labels r
//                    has in common with one of them, donor = the FIRST row that attains it; without such a row, or with m = 0
//                    (nothing to read from it), donor = -1.
//                    Row r computes the cells with u >= m(r): T (U + 1 - m) lattice rows; the cells with u < m(r) are the donor's,
//                    and the donor's own donor's where u < m(donor).  donor(r) < r, so a chain ends after at most 63 steps.
#pragma once
#include <stdint.h>

#include "../../include/rs_asr.h"

#if defined(__HIPCC__)
#define RS_ROWS_HD __host__ __device__ inline
#else
#define RS_ROWS_HD inline
#endif

enum { RS_ROWS_OK = 0, RS_ROWS_BAD_UTT = 1, RS_ROWS_DECREASE = 2, RS_ROWS_GROUP = 4 };
enum { RS_ROWS_NO_LATTICE = -1, RS_ROWS_BAD = -2 };

// what row_utt[r] does wrong, looking at the rows before it only (0 for a skipped row): every index a caller derives from row_utt
// is safe once this returned 0 for every row
RS_ROWS_HD int rs_align_rows_check_row(const int32_t* row_utt, int B, int r) {
    const int utt = row_utt[r];
    if (utt == -1) return RS_ROWS_OK;
    if (utt < -1 || utt >= B) return RS_ROWS_BAD_UTT;
    int count = 1;
    for (int q = r - 1; q >= 0; --q) {
        const int v = row_utt[q];
        if (v == -1) continue;
        if (v > utt) return RS_ROWS_DECREASE;
        if (v < utt) break;                                 // (a bad entry below -1 is reported by its own row)
        if (++count > RS_ALIGN_ROWS_PER_UTT_MAX) return RS_ROWS_GROUP;
    }
    return RS_ROWS_OK;
}

// U of a text that has a lattice on T frames; RS_ROWS_NO_LATTICE for the empty alignment (T = 0, U = 0) and an infeasible text;
// RS_ROWS_BAD for a count outside 0..u_cap, an id outside the vocabulary or the blank in the text
RS_ROWS_HD int rs_align_rows_lattice_u(int n, const int32_t* ids_row, int u_cap, int V, int blank, int T, int one_per_frame) {
    if (n < 0 || n > u_cap) return RS_ROWS_BAD;
    for (int u = 0; u < n; ++u) {
        const int id = ids_row[u];
        if (id < 0 || id >= V || id == blank) return RS_ROWS_BAD;
    }
    if (T <= 0 || (one_per_frame && n > T)) return RS_ROWS_NO_LATTICE;
    return n;
}

// m and donor of row r, which has a lattice (lat_u[r] >= 0); row_utt passed rs_align_rows_check_row on every row
RS_ROWS_HD void rs_align_rows_share(const int32_t* row_utt, const int32_t* lat_u, const int32_t* ids, int u_cap, int r, int* m,
                                    int* donor) {
    const int utt = row_utt[r], U = lat_u[r];
    const int32_t* mine = ids + (size_t)r * u_cap;
    int best = 0, from = -1;
    for (int q = r - 1; q >= 0; --q) {
        const int v = row_utt[q];
        if (v == -1) continue;
        if (v != utt) break;
        const int Uq = lat_u[q];
        if (Uq < 0) continue;                               // skipped above; bad, empty or infeasible: never a donor
        const int32_t* theirs = ids + (size_t)q * u_cap;
        const int most = U < Uq ? U : Uq;
        int c = 0;
        while (c < most && mine[c] == theirs[c]) ++c;
        if (c >= best) { best = c; from = q; }              // walking down: the last row kept is the first that attains it
    }
    *m = from < 0 ? 0 : best;
    *donor = best > 0 ? from : -1;                          // a row that shares no label gives nothing: no donor
}
