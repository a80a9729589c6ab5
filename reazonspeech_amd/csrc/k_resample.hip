// k_resample.hip — norm_audio on the device (rs_resample): polyphase resampling of every channel's mean to the model's rate.
//
// The filter is the host path's (nemo/asr/audio.py: _hq_filter); runtime/resample.py: plan() lays it out phase-major,
//   table[p][j] = up * h[p + j * up]     f32 [up][Jp], Jp = ceil(numtaps / up) rounded up to a multiple of 4, zero beyond numtaps
// and the output is scipy.signal.resample_poly's, cut to librosa's length:
//   n_out = ceil(L * up / down),   y[n] = sum_m x[m] * up * h[half + n * down - m * up],   half = (numtaps - 1) / 2.
// With c = half + n * down, p = c mod up and q = c div up this is  y[n] = sum_{j < Jp} x[q - j] * table[p][j]  (x = 0 outside the row).
//
// Form: a float32 VALU FIR, one fmaf chain per output in increasing j.  A thread owns ONE phase: it computes the I outputs
// n = nb + s + i * S of its tile (S = a multiple of `up` of about 256, so n mod up — hence p — is the same for all I) and reads its
// table row once, four taps per 16-byte load, for all of them.  The samples of a tile are staged through LDS once, as the mean of
// the channels (the mean is taken before the filter: one filter per row instead of one per channel; an impulse times a tap stays
// exact, and the error bound of tests/test_gpu_resample.py covers either order).  Window i of a workgroup holds the samples the
// outputs nb + s + i * S of its 256 residues s need: at most 255 * down / up + 2 + Jp floats.
//
// Index arithmetic: the tile origin nb is a multiple of S, hence of `up`, so nb * down / up = (nb / up) * down is exact and kept in
// 64 bits; everything else is relative to it.  Tiles start at each row's own first sample: a row's bits do not depend on the other
// rows of the launch.  One workgroup per (tile, slice of 256 residues, row), of as many waves as its residues fill (44.1 kHz:
// S = 160, three waves); it also writes the zeros of its part of the row beyond n_out, and the first one the zeros in front of
// out_offset and out_lens[b].
#include "rs_common.h"

namespace {

constexpr int RSMP_THREADS = 256;
constexpr int RSMP_LDS_FLOATS = 16384;        // 64 KiB of LDS per workgroup: no opt-in needed

template <int I>
__global__ __launch_bounds__(RSMP_THREADS) void resample_kernel(const float* __restrict__ x, const int64_t* __restrict__ row_off,
                                                                const int32_t* __restrict__ row_len, int channels,
                                                                const float* __restrict__ table, int up, int down, int half, int Jp, int S,
                                                                int Wi, float* __restrict__ out, long long out_pitch, int out_offset,
                                                                int32_t* __restrict__ out_lens) {
    extern __shared__ __attribute__((aligned(16))) float win[];          // [I][Wi]
    const int b = blockIdx.z, t = threadIdx.x;
    const long long L = row_len[b] > 0 ? row_len[b] : 0;
    const long long n_out = (L * up + down - 1) / down;
    float* orow = out + (long long)b * out_pitch;
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int c = t; c < out_offset; c += (int)blockDim.x) orow[c] = 0.0f;
        if (t == 0) out_lens[b] = (int32_t)(n_out < 0x7fffffffLL ? n_out : 0x7fffffffLL);
    }
    const long long nb = (long long)blockIdx.x * S * I;                  // first output of the tile: a multiple of S, hence of up
    const int s_lo = blockIdx.y * RSMP_THREADS, s = s_lo + t;
    const bool active = s < S;
    const long long step = (long long)(S / up) * down;                  // samples between the windows of outputs S apart
    const long long q_lo = (half + (long long)s_lo * down) / up;        // relative to qb
    int i_live = 0;                                                      // windows that hold an output of the row (uniform over the workgroup)
#pragma unroll
    for (int i = 0; i < I; ++i) i_live += nb + s_lo + (long long)i * S < n_out ? 1 : 0;
    float acc[I];
#pragma unroll
    for (int i = 0; i < I; ++i) acc[i] = 0.0f;
    if (i_live > 0) {
        const long long qb = (nb / up) * down;
        const float* xrow = x + row_off[b];
        const float n_ch = (float)channels;
        for (int i = 0; i < i_live; ++i) {
            const long long m0 = qb + q_lo + i * step - (Jp - 1);        // sample held by win[i][0]
            for (int idx = t; idx < Wi; idx += (int)blockDim.x) {
                const long long m = m0 + idx;
                float v = 0.0f;
                if (m >= 0 && m < L) {
                    v = xrow[m];
                    for (int c = 1; c < channels; ++c) v += xrow[c * L + m];
                    if (channels > 1) v = v / n_ch;
                }
                win[i * Wi + idx] = v;
            }
        }
        __syncthreads();
        if (active) {
            const long long c0 = half + (long long)s * down;
            const int p = (int)(c0 % up);
            const int base = (Jp - 1) + (int)(c0 / up - q_lo);           // win[i][base - j] = x[q_i - j]; base - j >= 0, base < Wi
            const float* trow = table + (size_t)p * Jp;
            for (int j = 0; j < Jp; j += 4) {
                const f32x4_t tv = *reinterpret_cast<const f32x4_t*>(trow + j);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                    for (int i = 0; i < I; ++i) acc[i] = fmaf(win[i * Wi + base - j - jj], tv[jj], acc[i]);
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const long long n = nb + s + (long long)i * S;
            const long long col = out_offset + n;
            if (col < out_pitch) orow[col] = (i < i_live && n < n_out) ? acc[i] : 0.0f;
        }
    }
}

}  // namespace

int rs_resample_impl(rs_ctx* ctx, const float* x, const int64_t* row_off, const int32_t* row_len, int B, int channels, const float* table,
                     int up, int down, int numtaps, float* out, long long out_pitch, int out_offset, int32_t* out_lens, hipStream_t s) {
    const int half = (numtaps - 1) / 2;
    const int Jp = ((numtaps + up - 1) / up + 3) / 4 * 4;
    const int S = up <= RSMP_THREADS ? up * (RSMP_THREADS / up) : up;
    const long long Wi = 255LL * down / up + 2 + Jp;
    if (Wi > RSMP_LDS_FLOATS)
        return rs_fail(ctx, RS_EINVAL, "resample: %d/%d with %d taps needs a window of %lld samples per workgroup, more than the %d that fit",
                       up, down, numtaps, Wi, RSMP_LDS_FLOATS);
    const int fit = (int)(RSMP_LDS_FLOATS / Wi);
    const int I = fit >= 8 ? 8 : fit >= 4 ? 4 : fit >= 2 ? 2 : 1;
    const long long tiles = (out_pitch - out_offset + (long long)S * I - 1) / ((long long)S * I);
    if (tiles > 0x7fffffffLL) return rs_fail(ctx, RS_EINVAL, "resample: out_pitch %lld is too long for one launch", out_pitch);
    const size_t lds = (size_t)I * Wi * sizeof(float);
    const int threads = S < RSMP_THREADS ? (S + 63) / 64 * 64 : RSMP_THREADS;     // no wave without a residue
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        const dim3 grid((unsigned)(tiles > 0 ? tiles : 1), (unsigned)((S + RSMP_THREADS - 1) / RSMP_THREADS), (unsigned)nb);
#define RS_RSMP_LAUNCH(II)                                                                                                              \
    hipLaunchKernelGGL(resample_kernel<II>, grid, dim3(threads), lds, s, x, row_off + b0, row_len + b0, channels, table, up, down, \
                       half, Jp, S, (int)Wi, out + (long long)b0 * out_pitch, out_pitch, out_offset, out_lens + b0)
        if (I == 8) RS_RSMP_LAUNCH(8);
        else if (I == 4) RS_RSMP_LAUNCH(4);
        else if (I == 2) RS_RSMP_LAUNCH(2);
        else RS_RSMP_LAUNCH(1);
#undef RS_RSMP_LAUNCH
        RS_CHECK_LAUNCH(ctx, "resample");
    }
    return RS_OK;
}
