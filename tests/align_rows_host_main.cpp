// Stand-alone driver of reazonspeech_amd/csrc/rs_align_rows_plan.h for tests/test_rnnt_align_rows_host.py (built with g++, once plain
// and once under the host sanitizers).  Reads groups from the file named by argv[1], one per block:
//   B R u_cap V blank one_per_frame
//   T of the B utterances | row_utt of the R rows | n_ids of the R rows | ids, R x u_cap
// and walks them as the plan kernel of csrc/k_rnnt_align.hip does: row_utt first, then the rows, then m and donor.  Every array
// lives in a heap block of exactly its size, so a plan that reads past one is caught by AddressSanitizer.  Prints per block
//   "err <code>"                                    and, when the code is 0,
//   "row <r> <lat_u> <m> <donor> <owned rows>"      for every row
//   "stats <computed> <without sharing>"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../reazonspeech_amd/csrc/rs_align_rows_plan.h"

static bool read_ints(FILE* f, std::vector<int32_t>& v, size_t n) {
    v.assign(n, 0);
    v.shrink_to_fit();
    for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%d", &v[i]) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    for (;;) {
        int B, R, u_cap, V, blank, one;
        if (fscanf(f, "%d %d %d %d %d %d", &B, &R, &u_cap, &V, &blank, &one) != 6) break;
        if (B < 0 || R < 0 || u_cap < 0) return 2;
        std::vector<int32_t> T, row_utt, n_ids, ids;
        if (!read_ints(f, T, B) || !read_ints(f, row_utt, R) || !read_ints(f, n_ids, R) || !read_ints(f, ids, (size_t)R * u_cap)) return 2;
        int err = 0;
        for (int r = 0; r < R; ++r) err |= rs_align_rows_check_row(row_utt.data(), B, r);
        printf("err %d\n", err);
        if (err) continue;
        std::vector<int32_t> lat_u(R, -1);
        lat_u.shrink_to_fit();
        for (int r = 0; r < R; ++r) {
            if (row_utt[r] < 0) continue;
            const int t = T[row_utt[r]] > 0 ? T[row_utt[r]] : 0;
            const int lu = rs_align_rows_lattice_u(n_ids[r], ids.data() + (size_t)r * u_cap, u_cap, V, blank, t, one);
            lat_u[r] = lu >= 0 ? lu : -1;
        }
        long long computed = 0, full = 0;
        for (int r = 0; r < R; ++r) {
            int m = 0, donor = -1;
            long long owned = 0;
            if (lat_u[r] >= 0) {
                rs_align_rows_share(row_utt.data(), lat_u.data(), ids.data(), u_cap, r, &m, &donor);
                if (donor >= r || m > lat_u[r] || (donor >= 0 && (row_utt[donor] != row_utt[r] || lat_u[donor] < m))) return 3;
                const long long t = T[row_utt[r]];
                owned = t * (lat_u[r] + 1 - m);
                full += t * (lat_u[r] + 1);
            }
            computed += owned;
            printf("row %d %d %d %d %lld\n", r, lat_u[r], m, donor, owned);
        }
        printf("stats %lld %lld\n", computed, full);
    }
    fclose(f);
    return 0;
}
