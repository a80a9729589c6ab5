// k_fft512.h — the 512-point register FFT shared by the log-mel front-end (k_frontend.hip) and the avsr log filterbank
// (k_avsr_features.hip): device functions only, everything a wave touches in LDS is its own.
//
// One wave transforms TWO real frames per 512-point complex FFT (frame t in the real part, t+1 in the
// imaginary part; the two real spectra are separated afterwards: X_a[k] = (Z[k] + conj Z[N-k]) / 2,
// X_b[k] = (Z[k] - conj Z[N-k]) / 2i).  The FFT is 512 = 8 x 8 x 8 (Cooley-Tukey): every lane holds eight complex values
// and runs three 8-point DFTs in registers, with two transposes through the wave's own LDS buffer between them —
// three LDS round trips per transform where a radix-2 in-LDS FFT makes nine (that version spent its time in LDS: 51 %
// bank conflicts, profiles/r02z_pmc_per_kernel.txt).  Layouts (in complex slots; a ds_*_b64 serves 32 lanes per cycle,
// conflict-free when their slots differ mod 32):
//   n = l + 64 k:  lane l, element k  -- DFT over k -> y[l][k1], * W512^(l k1) -> slot k1 * 68 + l
//   lane (k1 = j & 7, l2 = j >> 3) reads y[l2 + 8 l1][k1] -- DFT over l1 -> z[k1][l2][m1], * W64^(l2 m1)
//                                                                         -> slot m1 * 64 + ((l2 * 8 + k1 + 8 m1) & 63)
//   lane (k1, m1 = j >> 3) reads z[k1][.][m1] -- DFT over l2 -> Z[k1 + 8 (m1 + 8 m2)] -> slot j + 64 m2 (natural order)
// The steps are separated by wave-level fences, not workgroup barriers.
#pragma once
#include <hip/hip_runtime.h>

constexpr int FFT512_N = 512;
constexpr int FFT512_NBIN = 257;
constexpr int FFT512_BUF = 8 * 68;      // complex slots of one wave's transpose buffer

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// forward 8-point DFT of eight complex values in registers (three radix-2 decimation-in-frequency stages), natural order out
__device__ __forceinline__ void dft8(float2 (&a)[8]) {
    constexpr float S = 0.70710678118654752f;
    float2 b[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        b[j] = make_float2(a[j].x + a[j + 4].x, a[j].y + a[j + 4].y);
        b[j + 4] = make_float2(a[j].x - a[j + 4].x, a[j].y - a[j + 4].y);
    }
    b[5] = make_float2(S * (b[5].x + b[5].y), S * (b[5].y - b[5].x));          // * W8^1 = (1 - i) / sqrt 2
    b[6] = make_float2(b[6].y, -b[6].x);                                         // * W8^2 = -i
    b[7] = make_float2(S * (b[7].y - b[7].x), -S * (b[7].x + b[7].y));          // * W8^3 = (-1 - i) / sqrt 2
    float2 c[8];
#pragma unroll
    for (int h = 0; h < 8; h += 4) {
        c[h + 0] = make_float2(b[h].x + b[h + 2].x, b[h].y + b[h + 2].y);
        c[h + 2] = make_float2(b[h].x - b[h + 2].x, b[h].y - b[h + 2].y);
        c[h + 1] = make_float2(b[h + 1].x + b[h + 3].x, b[h + 1].y + b[h + 3].y);
        const float2 d = make_float2(b[h + 1].x - b[h + 3].x, b[h + 1].y - b[h + 3].y);
        c[h + 3] = make_float2(d.y, -d.x);                                       // * -i
    }
    a[0] = make_float2(c[0].x + c[1].x, c[0].y + c[1].y); a[4] = make_float2(c[0].x - c[1].x, c[0].y - c[1].y);
    a[2] = make_float2(c[2].x + c[3].x, c[2].y + c[3].y); a[6] = make_float2(c[2].x - c[3].x, c[2].y - c[3].y);
    a[1] = make_float2(c[4].x + c[5].x, c[4].y + c[5].y); a[5] = make_float2(c[4].x - c[5].x, c[4].y - c[5].y);
    a[3] = make_float2(c[6].x + c[7].x, c[6].y + c[7].y); a[7] = make_float2(c[6].x - c[7].x, c[6].y - c[7].y);
}

__device__ __forceinline__ void fft512_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// W512^j = (cos, -sin)(2 pi j / 512) for j in [0, 512): the table `tw` (LDS, 256 entries) holds the first half, the second is
// its negation
__device__ __forceinline__ float2 fft512_w(const float2* tw, int j) {
    const float2 w = tw[j & 255];
    return (j & 256) ? make_float2(-w.x, -w.y) : w;
}

// v[k] = (sample lane + 64 k of frame a, of frame b) on entry; on return z[0 .. 511] holds the complex spectrum in natural order
// (z: the wave's own FFT512_BUF slots of LDS).  A circular shift of the input only changes the phase, so a frame's samples sit
// at n = 0 .. win - 1 directly.
__device__ __forceinline__ void fft512_pair(float2 (&v)[8], float2* z, const float2* tw, int lane) {
    const int k1 = lane & 7, hi = lane >> 3;              // (k1, l2) in the second step, (k1, m1) in the third
    dft8(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q * 68 + lane] = q ? cmul(v[q], fft512_w(tw, lane * q)) : v[q];
    fft512_wave_sync();
    // ---- step 2: DFT over l1 for (k1, l2)
#pragma unroll
    for (int l1 = 0; l1 < 8; ++l1) v[l1] = z[k1 * 68 + hi + 8 * l1];
    fft512_wave_sync();                                    // every lane has its eight values before the buffer is rewritten
    dft8(v);
#pragma unroll
    for (int m1 = 0; m1 < 8; ++m1)
        z[m1 * 64 + ((hi * 8 + k1 + 8 * m1) & 63)] = m1 ? cmul(v[m1], fft512_w(tw, 8 * hi * m1)) : v[m1];
    fft512_wave_sync();
    // ---- step 3: DFT over l2 for (k1, m1): Z[k1 + 8 (m1 + 8 m2)] = natural slot lane + 64 m2
#pragma unroll
    for (int l2 = 0; l2 < 8; ++l2) v[l2] = z[hi * 64 + ((l2 * 8 + k1 + 8 * hi) & 63)];
    fft512_wave_sync();
    dft8(v);
#pragma unroll
    for (int m2 = 0; m2 < 8; ++m2) z[lane + 64 * m2] = v[m2];
    fft512_wave_sync();
}

// split the two real spectra of a transformed pair: |X_a[k]|^2 -> pa[k], |X_b[k]|^2 -> pb[k] for the bins 0 .. 256
__device__ __forceinline__ void fft512_split_power(const float2* z, float* pa, float* pb, int lane) {
    for (int k = lane; k < FFT512_NBIN; k += 64) {
        const float2 zk = z[k], zn = z[(FFT512_N - k) & (FFT512_N - 1)];
        const float ar = 0.5f * (zk.x + zn.x), ai = 0.5f * (zk.y - zn.y);
        const float br = 0.5f * (zk.y + zn.y), bi = 0.5f * (zn.x - zk.x);
        pa[k] = ar * ar + ai * ai;
        pb[k] = br * br + bi * bi;
    }
    fft512_wave_sync();
}
