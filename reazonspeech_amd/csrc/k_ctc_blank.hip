// k_ctc_blank.hip — where to cut a long recording, for a whole batch of windows on the device (rs_ctc_find_blank): a restatement of
// espnet/asr/ctc.py: find_blank(), which restates the reference's per-frame scan (pkg/espnet-asr/src/ctc.py:29-58).
//
//   ctc_find_blank_kernel   one wavefront per window.  A step takes 64 frames: each lane compares its frame's blank posterior with
//     the threshold in float32 (as numpy compares a float32 array with a Python float) and a 64-bit ballot of that predicate IS the
//     run structure of the step.  The mask is wave-uniform, so the walk over it — count-trailing-zeros on the mask for the first
//     frame of a run, on its complement for the first frame after it — is scalar work every lane repeats.  A run that is still
//     open at the end of a step is carried into the next one; one that is open after the last frame is dropped (the reference
//     only records a stretch when a non-silent frame closes it).
//     frame -> sample   (int64)((double)idx / (double)(T + 1) * (double)n): one double division, one double multiplication,
//                       truncation — Python's `int(idx / (frames + 1) * nsamples)`.  The file is built with -ffp-contract=off.
//     winner            the first candidate of the greatest end - start among those whose start sample is > 0, if that length is
//                       > 0; otherwise (n, n).
//   Frames past enc_lens[b] are never loaded.  A row whose length lies outside 0..tp_max writes (-1, -1) and reads nothing.
#include "rs_common.h"

namespace {

constexpr int BLANK_WAVE = 64;

__device__ __forceinline__ long long frame_to_sample(int idx, int T, int n) {
    const double q = (double)idx / (double)(T + 1);
    return (long long)(q * (double)n);
}

__global__ __launch_bounds__(BLANK_WAVE) void ctc_find_blank_kernel(const float* __restrict__ blank_prob, const int32_t* __restrict__ enc_lens,
                                                                    const int32_t* __restrict__ n_samples, int tp_max, float threshold,
                                                                    int32_t* __restrict__ cuts) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = enc_lens[b];
    int32_t* out = cuts + (size_t)b * 2;
    if (T < 0 || T > tp_max) {                                  // (uniform over the wavefront)
        if (lane == 0) { out[0] = -1; out[1] = -1; }
        return;
    }
    const int n = n_samples[b];
    const float* col = blank_prob + (size_t)b * tp_max;
    long long best_begin = n, best_end = n, best_len = 0;
    int open_first = -1;                                        // first frame of a run that reached the end of the previous step
    for (int base = 0; base < T; base += BLANK_WAVE) {
        const int nv = T - base < BLANK_WAVE ? T - base : BLANK_WAVE;
        bool silent = false;
        if (lane < nv) silent = col[base + lane] > threshold;
        const unsigned long long m = __ballot(silent);          // lanes past nv vote 0: a run never extends past the last frame here
        int pos = 0;
        while (pos < BLANK_WAVE) {
            int first;
            if (open_first >= 0) {
                first = open_first;                             // the carried run goes on at lane 0 (or ends right there)
            } else {
                const unsigned long long rest = m >> pos << pos;
                if (rest == 0) break;
                pos = __builtin_ctzll(rest);
                first = base + pos;
            }
            const unsigned long long gaps = ~m >> pos << pos;
            const int z = gaps ? __builtin_ctzll(gaps) : BLANK_WAVE;
            if (z >= nv) {                                      // silent up to the step's last frame: open (dropped after the last step)
                open_first = first;
                break;
            }
            open_first = -1;
            const long long begin = frame_to_sample(first, T, n), end = frame_to_sample(base + z, T, n);
            if (begin > 0 && end - begin > best_len) { best_len = end - begin; best_begin = begin; best_end = end; }
            pos = z + 1;                                        // frame z is not silent: the next run begins after it
        }
    }
    if (lane == 0) { out[0] = (int32_t)best_begin; out[1] = (int32_t)best_end; }
}

}  // namespace

int rs_ctc_find_blank_impl(rs_ctx* ctx, const float* blank_prob, const int32_t* enc_lens, const int32_t* n_samples, int B, int tp_max,
                           float threshold, int32_t* cuts, hipStream_t s) {
    hipLaunchKernelGGL(ctc_find_blank_kernel, dim3(B), dim3(BLANK_WAVE), 0, s, blank_prob, enc_lens, n_samples, tp_max, threshold, cuts);
    RS_CHECK_LAUNCH(ctx, "ctc_find_blank");
    return RS_OK;
}
