// k_avsr_features.hip — AVHubertFeatureExtractor on the device (rs_avsr_logfbank, rs_avsr_pixels): raw 16 kHz samples and uint8
// mouth crops in, the encoder's `input_values` / `pixel_values` out.  The host half (the mel table, the grey-level table, the crop
// window, the frame index) is reazonspeech_amd/runtime/avsr_features.py: plan().
//
// Audio (avsr_logfbank_stack_ln_kernel) — python_speech_features.logfbank with its defaults, the stacker and the per-row LayerNorm
// of reazonspeech_amd/avsr/feature_extraction.py, in float32:
//   s'[0] = s[0], s'[i] = s[i] - 0.97 s[i-1];  frame f = s'[160 f .. 160 f + 400), zero beyond the clip;
//   frames = 1 if n <= 400 else 1 + ceil((n - 400) / 160);  E[f][m] = sum_k fb[m][k] |rfft512(frame f)[k]|^2 / 512;
//   L[f][m] = logf(E == 0 ? 2.220446e-16 : E);  stacked row r = L[stack r .. stack r + stack) (frames >= `frames` are zeros,
//   not log(eps));  LayerNorm over the 26 * stack features of the row (two-pass, biased variance, eps 1e-5, no affine).
// One WAVE produces one stacked row: ceil(stack / 2) transforms of two real frames each (k_fft512.h), the 257-bin spectra and the
// row's log energies only in the wave's own LDS; a workgroup of four waves stages the pre-emphasised samples under its four rows
// once.  A row is computed from its clip's samples alone, by one wave, whatever else the launch holds: its bits do not depend on
// the other rows.  The mean is taken around the row's first feature (mu = x0 + mean(x - x0)): a row of equal features — all-zero
// audio: 26 * stack times log(eps) — is centred to exact zeros, where a plain float32 sum of 104 equal terms is not their multiple.
//
// Video (avsr_pixels_kernel): out[b][t] = lut[grey(frame frame_idx[b][t])[top .. top + crop)[left .. left + crop)], one workgroup
// per output frame, four pixels per lane and store (16 bytes), the four uint8 read as aligned 32-bit words and shifted into place
// when `left` (or three bytes per BGR pixel) leaves them unaligned.  Write-bound: 4 * crop^2 bytes out per crop^2 (3 crop^2) in.
#include "rs_common.h"
#include "k_fft512.h"

namespace {

constexpr int FB_NFILT = RS_AVSR_FBANK_FILTERS;   // 26
constexpr int FB_MAXW = RS_AVSR_FBANK_MAXW;       // columns of the banded filter table
constexpr int FB_WIN = 400, FB_HOP = 160;         // 25 ms / 10 ms at 16 kHz
constexpr int FB_WAVES = 4;                       // stacked rows per workgroup
constexpr int FB_MAX_STACK = 8;
constexpr int FB_SPAN_MAX = (FB_WAVES * FB_MAX_STACK - 1) * FB_HOP + FB_WIN;
constexpr float FB_PREEMPH = 0.97f;
constexpr float FB_EPS = 2.220446049250313e-16f;  // float64 machine epsilon, 2^-52: exact in float32
constexpr float FB_LN_EPS = 1e-5f;

__global__ __launch_bounds__(64 * FB_WAVES) void avsr_logfbank_stack_ln_kernel(
    const float* __restrict__ audio, const int64_t* __restrict__ row_off, const int32_t* __restrict__ row_len, int T, int stack,
    int normalize, const float* __restrict__ twiddle, const int32_t* __restrict__ fb_idx, const float* __restrict__ fb_w,
    float* __restrict__ out) {
    __shared__ float2 buf[FB_WAVES][FFT512_BUF];
    __shared__ float pw[FB_WAVES][2][FFT512_NBIN + 3];
    __shared__ float2 tw[FFT512_N / 2];
    __shared__ float ys[FB_SPAN_MAX];
    __shared__ float feat[FB_WAVES][FB_NFILT * FB_MAX_STACK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int n = row_len[b];                                            // < 0: a clip without audio
    const int frames = n < 0 ? 0 : (n <= FB_WIN ? 1 : 1 + (n - FB_WIN + FB_HOP - 1) / FB_HOP);
    const int rows = (frames + stack - 1) / stack;
    const int F = FB_NFILT * stack;
    const int r0 = blockIdx.x * FB_WAVES, r = r0 + wave;
    float* orow = out + ((size_t)b * T + r) * F;
    if (r0 >= rows) {                                                    // block-uniform: nothing but zero rows
        if (r < T)
            for (int i = lane; i < F; i += 64) orow[i] = 0.0f;
        return;
    }
    tw[threadIdx.x] = reinterpret_cast<const float2*>(twiddle)[threadIdx.x];      // 256 threads, 256 twiddles
    const float* a = audio + row_off[b];
    const int f0 = r0 * stack;                                           // first frame of the workgroup
    const long long i_base = (long long)f0 * FB_HOP;
    const int span = (FB_WAVES * stack - 1) * FB_HOP + FB_WIN;           // <= FB_SPAN_MAX for stack <= FB_MAX_STACK
    for (int idx = threadIdx.x; idx < span; idx += 64 * FB_WAVES) {
        const long long i = i_base + idx;
        float y = 0.0f;
        if (i < n) y = i >= 1 ? fmaf(-FB_PREEMPH, a[i - 1], a[i]) : a[0];
        ys[idx] = y;
    }
    __syncthreads();
    if (r >= T) return;                                                  // wave-uniform; no workgroup barrier below
    if (r >= rows) {
        for (int i = lane; i < F; i += 64) orow[i] = 0.0f;
        return;
    }
    float2* z = buf[wave];
    float* fe = feat[wave];
    for (int fi = 0; fi < stack; fi += 2) {
        const int t = r * stack + fi;
        if (t >= frames) {                                               // wave-uniform: frames past the clip contribute zeros
            for (int i = lane; i < 2 * FB_NFILT; i += 64)
                if (fi * FB_NFILT + i < F) fe[fi * FB_NFILT + i] = 0.0f;
            fft512_wave_sync();
            continue;
        }
        const bool two = fi + 1 < stack && t + 1 < frames;               // an odd last frame is paired with zeros
        const float* fr = ys + (t - f0) * FB_HOP;
        float2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = lane + 64 * k;
            const bool in = s < FB_WIN;
            v[k] = make_float2(in ? fr[s] : 0.0f, in && two ? fr[FB_HOP + s] : 0.0f);
        }
        fft512_pair(v, z, tw, lane);
        fft512_split_power(z, pw[wave][0], pw[wave][1], lane);
        for (int idx = lane; idx < 2 * FB_NFILT; idx += 64) {
            const int f = idx >= FB_NFILT, m = idx - f * FB_NFILT;
            if (fi + f < stack) {
                float e = 0.0f;
                if (t + f < frames) {
                    int k0 = fb_idx[2 * m], cnt = fb_idx[2 * m + 1];
                    k0 = min(max(k0, 0), FFT512_NBIN);
                    cnt = min(min(max(cnt, 0), FB_MAXW), FFT512_NBIN - k0);
                    const float* w = fb_w + m * FB_MAXW;
                    float acc = 0.0f;
                    for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], pw[wave][f][k0 + j], acc);
                    acc *= 1.0f / (float)FFT512_N;
                    e = logf(acc == 0.0f ? FB_EPS : acc);
                }
                fe[(fi + f) * FB_NFILT + m] = e;
            }
        }
        fft512_wave_sync();
    }
    // LayerNorm of the row (F <= 208 features: up to four per lane)
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = lane + 64 * q < F ? fe[lane + 64 * q] : 0.0f;
    if (normalize) {
        const float x0 = fe[0];
        const float inv = 1.0f / (float)F;
        float sm = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = lane + 64 * q < F ? x[q] - x0 : 0.0f;
            sm += x[q];
        }
        const float md = wave_sum(sm) * inv;
        float sq = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = lane + 64 * q < F ? x[q] - md : 0.0f;
            sq = fmaf(x[q], x[q], sq);
        }
        const float sd = sqrtf(wave_sum(sq) * inv + FB_LN_EPS);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = x[q] / sd;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < F) orow[lane + 64 * q] = x[q];
}

// four source bytes at byte offset `off` of a 4-byte aligned buffer of `total` bytes: two aligned words shifted into place; the last
// words of the buffer byte by byte
__device__ __forceinline__ uint32_t load_u8x4(const uint8_t* __restrict__ src, size_t off, size_t total) {
    const size_t a0 = off & ~(size_t)3;
    if (a0 + 8 <= total) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(src + a0);
        const uint32_t lo = w[0], hi = w[1];
        const int sh = (int)(off & 3) * 8;
        return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (off + k < total) v |= (uint32_t)src[off + k] << (8 * k);
    return v;
}

__device__ __forceinline__ uint32_t bgr2gray(uint32_t bl, uint32_t g, uint32_t rd) {
    return (1868u * bl + 9617u * g + 4899u * rd + 8192u) >> 14;         // OpenCV's 8-bit COLOR_BGR2GRAY
}

// grid (T, B), 256 threads: output frame (b, t)
template <int CH>
__global__ __launch_bounds__(256) void avsr_pixels_kernel(const uint8_t* __restrict__ src, long long n_frames, int H, int W,
                                                          const int32_t* __restrict__ frame_idx, int idx_pitch, int T, int crop, int top,
                                                          int left, const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float lut_s[256];
    const int b = blockIdx.y, t = blockIdx.x;
    const int fi = frame_idx[(size_t)b * idx_pitch + t];
    if (fi < -1) return;                                                 // a frame of another launch (another frame size)
    lut_s[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    float* o = out + ((size_t)b * T + t) * crop * crop;
    const bool blank = fi < 0 || fi >= n_frames;                         // padding / no video: grey level 0
    const size_t total = (size_t)n_frames * H * W * CH;
    const size_t fbase = blank ? 0 : (size_t)fi * H * W;                 // in pixels
    const int qpr = crop >> 2;                                           // 16-byte stores per row (crop % 4 == 0: rs_avsr_pixels)
    const int nq = crop * qpr;
    f32x4_t* o4 = reinterpret_cast<f32x4_t*>(o);                         // 16-byte aligned: out is, and crop^2 % 4 == 0
    const float z = lut_s[0];
    for (int q = threadIdx.x; q < nq; q += 256) {
        f32x4_t v = {z, z, z, z};
        if (!blank) {
            const int y = q / qpr, x = (q - y * qpr) * 4;
            const size_t px = fbase + (size_t)(top + y) * W + left + x;
            uint32_t g4;
            if (CH == 1) {
                g4 = load_u8x4(src, px, total);
            } else {
                const uint32_t w0 = load_u8x4(src, 3 * px, total), w1 = load_u8x4(src, 3 * px + 4, total),
                               w2 = load_u8x4(src, 3 * px + 8, total);
                g4 = bgr2gray(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255) |
                     bgr2gray(w0 >> 24, w1 & 255, (w1 >> 8) & 255) << 8 |
                     bgr2gray((w1 >> 16) & 255, w1 >> 24, w2 & 255) << 16 |
                     bgr2gray((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24) << 24;
            }
            v = f32x4_t{lut_s[g4 & 255], lut_s[(g4 >> 8) & 255], lut_s[(g4 >> 16) & 255], lut_s[g4 >> 24]};
        }
        o4[q] = v;
    }
}

}  // namespace

hipError_t rs_avsr_logfbank_launch(const float* audio, const int64_t* row_off, const int32_t* row_len, int B, int T, int stack, int normalize,
                                   const float* twiddle, const int32_t* fb_idx, const float* fb_w, float* out, hipStream_t s) {
    const int F = FB_NFILT * stack;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        const dim3 grid((unsigned)((T + FB_WAVES - 1) / FB_WAVES), (unsigned)nb);
        hipLaunchKernelGGL(avsr_logfbank_stack_ln_kernel, grid, dim3(64 * FB_WAVES), 0, s, audio, row_off + b0, row_len + b0, T, stack,
                           normalize, twiddle, fb_idx, fb_w, out + (size_t)b0 * T * F);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rs_avsr_pixels_launch(const uint8_t* frames, long long n_frames, int H, int W, int channels, const int32_t* frame_idx, int idx_pitch,
                                 int B, int T, int crop, int top, int left, const float* lut, float* out, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        const dim3 grid((unsigned)T, (unsigned)nb);
        const int32_t* idx = frame_idx + (size_t)b0 * idx_pitch;
        float* o = out + (size_t)b0 * T * crop * crop;
        if (channels == 1)
            hipLaunchKernelGGL(avsr_pixels_kernel<1>, grid, dim3(256), 0, s, frames, n_frames, H, W, idx, idx_pitch, T, crop, top, left, lut, o);
        else
            hipLaunchKernelGGL(avsr_pixels_kernel<3>, grid, dim3(256), 0, s, frames, n_frames, H, W, idx, idx_pitch, T, crop, top, left, lut, o);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
