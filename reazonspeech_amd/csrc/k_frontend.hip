// k_frontend.hip — log-mel front-end.
//
// [UPSTREAM] AudioToMelSpectrogramPreprocessor / FilterbankFeatures.forward:
//   pre-emphasis 0.97 -> STFT(n_fft 512, hann 400 centred in the frame, hop 160, center=True with
//   zero edge padding) -> |.|^2 -> Slaney mel (80 banded filters) -> log(x + 2^-24)
//   -> per-utterance, per-feature (mean, unbiased std) normalisation over the valid frames
//   -> zero the padding frames.
// pad_audio (pkg/nemo-asr/src/audio.py:70-83) is folded into the sample fetch: the kernel reads
// raw[i - pad_left] and everything outside [0, len) is 0.0, which is what np.pad would have stored.
//
// HBM-bound by construction: the audio is read once (each sample is touched by ~3 overlapping
// frames, served by L2), the 257-bin spectrum lives only in LDS, and 80 floats per frame go out.
// The 512-point FFT is an 8 x 8 x 8 register transform with two LDS transposes, two frames per wave; this is
// integer/float streaming work, deliberately NOT reshaped into a DFT GEMM.
#include "rs_common.h"
#include "k_fft512.h"

namespace {

constexpr int NFFT = FFT512_N;
constexpr int NBIN = FFT512_NBIN;
constexpr int FB_MAXW = 32;          // widest Slaney filter has 18 taps at 80 mels / 512 fft
constexpr int WAVES = 4;
constexpr int FRAMES_PER_WAVE = 4;   // frames per block = 16
constexpr int MAX_HOP = 256;         // the workgroup's span of the signal is staged in LDS: (frames per block - 1) * hop + n_fft samples
constexpr int SPAN_MAX = (WAVES * FRAMES_PER_WAVE - 1) * MAX_HOP + NFFT;

struct FrontParams {
    const float* audio; const int32_t* lens; float* raw; int32_t* n_frames;
    const float* window;   // [win_length]
    const float* twiddle;  // [256][2] cos, -sin of 2*pi*j/512
    const int32_t* fb_idx; // [n_mels][2] first bin, tap count
    const float* fb_w;     // [n_mels][FB_MAXW]
    int audio_stride, pad_left, pad_right, t_max, n_mels, win_length, hop;
    float preemph, log_guard;
    int kind;              // 0: NeMo (zero edge padding, floor(L / hop) frames, log(x + guard)); 1: ESPnet DefaultFrontend
                           // (reflect edge padding, 1 + floor(L / hop) frames, log(max(x, guard)); normalised by feat_mvn_kernel);
                           // 2: kaldi-native-fbank as sherpa-onnx configures it (reazonspeech.k2.asr): snip_edges = false — frame f
                           // covers samples [hop f + hop / 2 - win / 2, .. + win), edges REFLECTED (-1 -> 0, L -> L - 1) —, per frame:
                           // subtract the mean, x[i] -= preemph x[i - 1] (x[0] -= preemph x[0]), window, log(max(x, guard)); the
                           // features are written as they are (no normalisation)
};

__device__ __forceinline__ float fetch_sample(const float* __restrict__ a, int i, int pad_left, int len) {
    const int j = i - pad_left;
    return (j >= 0 && j < len) ? a[j] : 0.0f;
}

// The 512-point transform (two real frames per complex FFT, 8 x 8 x 8 in registers, wave-private LDS): k_fft512.h.
// Everything a wave touches in LDS is its own, so the steps are separated by wave-level fences, not workgroup
// barriers; the twiddles are staged once per workgroup.
//
// LEAN = false is the first form: every frame pair reads the filterbank (fb_idx, fb_w) from global memory inside the mel chain,
// and the staged span is sized for the largest hop.  LEAN = true keeps the transform, the staging rule and the mel chain as they
// are (same fmaf order, same logf: same bits) and changes where the operands wait:
//   - the filterbank is staged once per workgroup into LDS, tap-major with a row pitch of n_mels + 1 (the coalesced copy from
//     [mel][FB_MAXW] writes a column: pitch 81 spreads it over the banks; the mel stage reads along a row);
//   - a lane's items of the mel stage (frame of the pair, mel bin) are the same for every pair, so their first bin and tap count
//     are looked up once, and the tap loop runs to the wave's largest count with a select — a uniform trip count the compiler
//     unrolls, so the LDS reads of several taps are in flight together instead of one dependent global load per tap;
//   - the window sits in eight registers per lane (sample n = lane + 64 k), not in LDS;
//   - the span is dynamic LDS sized by the actual hop: 49 792 bytes per workgroup at hop 160 / 80 mels, three workgroups per
//     CU as before (the first form: 47 232), and its samples are asked for from HBM together, not one wait per element.
constexpr int MEL_PASSES = 4;        // 2 * n_mels <= 256 items over 64 lanes
template <bool LEAN>
__global__ __launch_bounds__(64 * WAVES) void logmel_kernel(FrontParams p) {
    __shared__ float2 buf[WAVES][FFT512_BUF];
    __shared__ float pw[WAVES][2][NBIN + 3];
    __shared__ float2 tw[NFFT / 2];
    __shared__ float ys_first[LEAN ? 1 : SPAN_MAX];
    __shared__ float win_first[LEAN ? 1 : NFFT];
    extern __shared__ float lean_lds[];              // LEAN: ys[span] | fbw_s[FB_MAXW][n_mels + 1]
    float* const ys = LEAN ? lean_lds : ys_first;
    float* const win_s = win_first;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int len = p.lens[b];
    const int Lp = len + p.pad_left + p.pad_right;       // padded length (reference: after pad_audio)
    const int n_valid = p.kind == 2 ? (Lp + p.hop / 2) / p.hop
                                    : Lp / p.hop + (p.kind == 1 ? 1 : 0);   // NeMo: floor((Lp + 2*(n_fft/2) - n_fft) / hop); ESPnet Stft keeps the last frame
    if (blockIdx.x == 0 && threadIdx.x == 0) p.n_frames[b] = n_valid;
    const float* a = p.audio + (size_t)b * p.audio_stride;
    if ((int)blockIdx.x * WAVES * FRAMES_PER_WAVE >= min(n_valid, p.t_max)) return;  // block-uniform
    tw[threadIdx.x] = reinterpret_cast<const float2*>(p.twiddle)[threadIdx.x];      // 256 threads, 256 twiddles
    // The padded, pre-emphasised signal under this workgroup's 16 frames goes through LDS once (coalesced loads; the
    // samples of a frame were fetched lane by lane before: 48 small loads per lane and transform) together with the
    // window, zero beyond its length.  Index i runs in the PADDED signal (reference: after pad_audio); everything
    // outside [0, Lp) is zero, and y[0] = x[0] has no predecessor.
    const int centre_off = (NFFT - p.win_length) / 2;     // 56: window centred in the 512 frame
    const int f0 = blockIdx.x * WAVES * FRAMES_PER_WAVE;
    const int i_base = p.kind == 2 ? f0 * p.hop + p.hop / 2 - p.win_length / 2 : f0 * p.hop - NFFT / 2 + centre_off;
    const int span = (WAVES * FRAMES_PER_WAVE - 1) * p.hop + NFFT;
    const int fb_pitch = p.n_mels + 1;
    float* const fbw_s = lean_lds + span;
    float wreg[8];                                    // LEAN: the window at n = lane + 64 k, zero beyond its length
    int it_m[MEL_PASSES], it_k0[MEL_PASSES], it_cnt[MEL_PASSES];     // LEAN: this lane's mel items (idx = lane + 64 q)
    int cnt_max = 0;
    if constexpr (LEAN) {                             // (the tables are in L2: asked for before the samples, they arrive under them)
#pragma unroll 5
        for (int e = threadIdx.x; e < p.n_mels * FB_MAXW; e += blockDim.x)       // fb_w[m][j] -> fbw_s[j][m]
            fbw_s[(e % FB_MAXW) * fb_pitch + e / FB_MAXW] = p.fb_w[e];
#pragma unroll
        for (int k = 0; k < 8; ++k) wreg[k] = lane + 64 * k < p.win_length ? p.window[lane + 64 * k] : 0.0f;
#pragma unroll
        for (int q = 0; q < MEL_PASSES; ++q) {
            const int idx = lane + 64 * q;
            const bool on = idx < 2 * p.n_mels;
            const int m = on ? idx - (idx >= p.n_mels ? p.n_mels : 0) : 0;
            it_m[q] = m;
            it_k0[q] = on ? p.fb_idx[2 * m] : 0;
            it_cnt[q] = on ? min(p.fb_idx[2 * m + 1], FB_MAXW) : 0;
            cnt_max = max(cnt_max, it_cnt[q]);
        }
    }
    auto padded_index = [&](int idx) -> int {           // element idx of the span -> index in the padded signal after the edge rule
        int i = i_base + idx;
        if (p.kind == 1 && Lp > 1) {                      // torch.stft(pad_mode="reflect"): x[-k] = x[k], x[L-1+k] = x[L-1-k]
            i = i < 0 ? -i : i;
            i = i >= Lp ? 2 * (Lp - 1) - i : i;
            i = i < 0 ? 0 : i;                            // (an utterance shorter than n_fft / 2: torch refuses it, clamp)
        }
        if (p.kind == 2 && Lp > 0) {                      // kaldi ExtractWindow: reflect without repeating the end sample, as often as needed
            for (int bounce = 0; bounce < 8 && (i < 0 || i >= Lp); ++bounce) i = i < 0 ? -i - 1 : 2 * Lp - 1 - i;
            i = i < 0 ? 0 : (i >= Lp ? Lp - 1 : i);
        }
        return i;
    };
    if constexpr (LEAN) {
        // The samples come from HBM for the first time.  A loop of "load, load, store" waits for memory once per element and
        // thread (a dozen times per workgroup); here the loads of STAGE_CHUNK elements per thread are issued together — from a
        // clamped address, without a branch around them — and the edge rule picks value or zero afterwards.
        constexpr int STAGE_CHUNK = 12;                   // 12 * 256 = 3072 elements: the whole span at hop 160
        for (int base = 0; base < span; base += STAGE_CHUNK * 64 * WAVES) {
            float r0[STAGE_CHUNK], r1[STAGE_CHUNK];
#pragma unroll
            for (int k = 0; k < STAGE_CHUNK; ++k) {
                const int j = padded_index(base + k * 64 * WAVES + (int)threadIdx.x) - p.pad_left;
                r0[k] = 0.0f; r1[k] = 0.0f;
                if (len > 0) {                            // (uniform; a[0] need not exist for an empty utterance)
                    r0[k] = a[min(max(j, 0), len - 1)];
                    if (p.kind != 2) r1[k] = a[min(max(j - 1, 0), len - 1)];
                }
            }
#pragma unroll
            for (int k = 0; k < STAGE_CHUNK; ++k) {
                const int idx = base + k * 64 * WAVES + (int)threadIdx.x;
                const int i = padded_index(idx), j = i - p.pad_left;
                float y = 0.0f;
                if (i >= 0 && i < Lp) {
                    const float x0 = (j >= 0 && j < len) ? r0[k] : 0.0f;
                    if (p.kind == 2) y = x0;
                    else y = i >= 1 ? x0 - p.preemph * ((j - 1 >= 0 && j - 1 < len) ? r1[k] : 0.0f) : x0;
                }
                if (idx < span) ys[idx] = y;
            }
        }
    } else
    for (int idx = threadIdx.x; idx < span; idx += blockDim.x) {
        int i = padded_index(idx);
        float y = 0.0f;
        if (i >= 0 && i < Lp) {
            const float x0 = fetch_sample(a, i, p.pad_left, len);
            if (p.kind == 2) y = x0;                      // DC removal and pre-emphasis are per FRAME (below)
            else y = i >= 1 ? x0 - p.preemph * fetch_sample(a, i - 1, p.pad_left, len) : x0;
        }
        ys[idx] = y;
    }
    if constexpr (LEAN) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt_max = max(cnt_max, __shfl_xor(cnt_max, off, 64));
        cnt_max = __builtin_amdgcn_readfirstlane(cnt_max);
    } else
        for (int idx = threadIdx.x; idx < NFFT; idx += blockDim.x) win_s[idx] = idx < p.win_length ? p.window[idx] : 0.0f;
    __syncthreads();
    const int frame_base = (blockIdx.x * WAVES + wave) * FRAMES_PER_WAVE;
    auto wave_sync = [&]() { fft512_wave_sync(); };
    // windowed, pre-emphasised sample n of frame t (0 for a frame past the utterance)
    auto sample = [&](int t, int n) -> float {
        if (t >= n_valid || t >= p.t_max) return 0.0f;
        return ys[(t - f0) * p.hop + n] * win_s[n];
    };
    auto sample_lean = [&](int t, int k) -> float {      // the same product with the window from its register
        if (t >= n_valid || t >= p.t_max) return 0.0f;
        return ys[(t - f0) * p.hop + lane + 64 * k] * wreg[k];
    };
    // kaldi: (x[n] - mean) - preemph (x[n - 1] - mean), the first sample against itself; mean over the frame's win_length samples
    auto frame_mean = [&](int t) -> float {
        if (t >= n_valid || t >= p.t_max) return 0.0f;
        float sm = 0.0f;
        for (int n = lane; n < p.win_length; n += 64) sm += ys[(t - f0) * p.hop + n];
        return wave_sum(sm) / (float)p.win_length;
    };
    auto sample_kaldi = [&](int t, int n, float mean) -> float {
        if (t >= n_valid || t >= p.t_max || n >= p.win_length) return 0.0f;
        const float* fr = ys + (t - f0) * p.hop;
        const float cur = fr[n] - mean, prev = fr[n > 0 ? n - 1 : 0] - mean;
        return (cur - p.preemph * prev) * win_s[n];
    };
    auto sample_kaldi_lean = [&](int t, int k, float mean) -> float {
        const int n = lane + 64 * k;
        if (t >= n_valid || t >= p.t_max || n >= p.win_length) return 0.0f;
        const float* fr = ys + (t - f0) * p.hop;
        const float cur = fr[n] - mean, prev = fr[n > 0 ? n - 1 : 0] - mean;
        return (cur - p.preemph * prev) * wreg[k];
    };

    for (int fi = 0; fi < FRAMES_PER_WAVE; fi += 2) {
        const int t = frame_base + fi;
        if (t >= n_valid || t >= p.t_max) break;          // wave-uniform
        float2* z = buf[wave];
        // ---- step 1: two frames, samples n = lane + 64 k.  A circular shift of the FFT input only changes the phase,
        // so the 400 samples sit at n = 0 .. 399 directly.
        float2 v[8];
        if constexpr (LEAN) {
            if (p.kind == 2) {
                const float m0 = frame_mean(t), m1 = frame_mean(t + 1);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = make_float2(sample_kaldi_lean(t, k, m0), sample_kaldi_lean(t + 1, k, m1));
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = make_float2(sample_lean(t, k), sample_lean(t + 1, k));
            }
        } else if (p.kind == 2) {
            const float m0 = frame_mean(t), m1 = frame_mean(t + 1);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = make_float2(sample_kaldi(t, lane + 64 * k, m0), sample_kaldi(t + 1, lane + 64 * k, m1));
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = make_float2(sample(t, lane + 64 * k), sample(t + 1, lane + 64 * k));
        }
        fft512_pair(v, z, tw, lane);
        // ---- split the two spectra, power of bins 0..256
        fft512_split_power(z, pw[wave][0], pw[wave][1], lane);
        // ---- banded mel filterbank + log: lane -> (frame of the pair, mel bin)
        if constexpr (LEAN) {
#pragma unroll
            for (int q = 0; q < MEL_PASSES; ++q) {
                if (64 * q >= 2 * p.n_mels) break;            // (uniform)
                const int idx = lane + 64 * q;
                const int f = idx >= p.n_mels, m = it_m[q], k0 = it_k0[q], cnt = it_cnt[q];
                const float* pwr = pw[wave][f];
                const float* wcol = fbw_s + m;
                float acc = 0.0f;
#pragma unroll 6
                for (int j = 0; j < cnt_max; ++j) {           // taps past this item's count are read (clamped) and not taken
                    const float next = fmaf(wcol[j * fb_pitch], pwr[min(k0 + j, NBIN - 1)], acc);
                    acc = j < cnt ? next : acc;
                }
                if (idx < 2 * p.n_mels && t + f < n_valid && t + f < p.t_max)
                    p.raw[((size_t)b * p.t_max + t + f) * p.n_mels + m] = p.kind >= 1 ? logf(fmaxf(acc, p.log_guard)) : logf(acc + p.log_guard);
            }
        } else
        for (int idx = lane; idx < 2 * p.n_mels; idx += 64) {
            const int f = idx >= p.n_mels, m = idx - f * p.n_mels;
            if (t + f < n_valid && t + f < p.t_max) {
                const int k0 = p.fb_idx[2 * m], cnt = p.fb_idx[2 * m + 1];
                const float* w = p.fb_w + m * FB_MAXW;
                float acc = 0.0f;
                for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], pw[wave][f][k0 + j], acc);
                p.raw[((size_t)b * p.t_max + t + f) * p.n_mels + m] = p.kind >= 1 ? logf(fmaxf(acc, p.log_guard)) : logf(acc + p.log_guard);
            }
        }
        wave_sync();
    }
}

// per utterance: mean / unbiased std over the valid frames, normalise, zero the padding.
// One workgroup of 1000 (+24 idle) threads per utterance; the [t][n_mels] block is walked as float4
// columns: thread i owns mel quad i % Q and rows i / Q + k * (1000 / Q), so its partial sums stay in
// registers and every pass is ~22 independent 16-byte loads per thread instead of 550 dependent
// 4-byte ones (the previous 256-thread version: 480 us, latency-bound).  Statistics are two-pass
// (mean, then sum of squared deviations) like torch's; passes 2 and 3 re-read the block from L2.
__global__ __launch_bounds__(1024) void feat_normalize_kernel(const float* __restrict__ raw,
                                                              const int32_t* __restrict__ n_frames, int t_max,
                                                              int n_mels, float eps, float* __restrict__ out) {
    __shared__ float4 red[1024];
    __shared__ float4 mean_s[32], rstd_s[32];
    const int b = blockIdx.x;
    const int n = min(n_frames[b], t_max);
    const int Q = n_mels >> 2;                       // float4 per row (n_mels % 4 == 0, Q <= 32)
    const int RG = 1000 / Q;                         // row groups walked in parallel
    const int tid = threadIdx.x;
    const int q = tid % Q, rg = tid / Q;
    const bool act = rg < RG;
    const float4* r4 = reinterpret_cast<const float4*>(raw + (size_t)b * t_max * n_mels);
    auto reduce_rows = [&](float4 v) -> float4 {     // sum over row groups; result valid in threads rg == 0
        red[tid] = act ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < Q) {
            for (int g = 0; g < RG; ++g) {
                const float4 x = red[g * Q + tid];
                acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
            }
        }
        return acc;
    };
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (act)
#pragma unroll 8
        for (int t = rg; t < n; t += RG) {
            const float4 x = r4[(size_t)t * Q + q];
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
    s = reduce_rows(s);
    if (tid < Q) {
        const float inv = 1.0f / (float)n;
        mean_s[tid] = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    }
    __syncthreads();
    const float4 mean = mean_s[q];
    float4 m2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (act)
#pragma unroll 8
        for (int t = rg; t < n; t += RG) {
            const float4 x = r4[(size_t)t * Q + q];
            const float a = x.x - mean.x, bb = x.y - mean.y, c = x.z - mean.z, d = x.w - mean.w;
            m2.x += a * a; m2.y += bb * bb; m2.z += c * c; m2.w += d * d;
        }
    m2 = reduce_rows(m2);
    if (tid < Q) {
        // n == 1: the unbiased variance is 0/0 (NaN in the reference stack too); emit zeros instead of
        // poisoning the encoder and the argmax
        const float dn = (float)(n - 1);
        rstd_s[tid] = n > 1 ? make_float4(1.0f / (sqrtf(m2.x / dn) + eps), 1.0f / (sqrtf(m2.y / dn) + eps),
                                          1.0f / (sqrtf(m2.z / dn) + eps), 1.0f / (sqrtf(m2.w / dn) + eps))
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const float4 rstd = rstd_s[q];
    float4* o4 = reinterpret_cast<float4*>(out + (size_t)b * t_max * n_mels);
    if (act)
#pragma unroll 8
        for (int t = rg; t < t_max; t += RG) {
            float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < n) {
                const float4 x = r4[(size_t)t * Q + q];
                y = make_float4((x.x - mean.x) * rstd.x, (x.y - mean.y) * rstd.y, (x.z - mean.z) * rstd.z,
                                (x.w - mean.w) * rstd.w);
            }
            o4[(size_t)t * Q + q] = y;
        }
}

// ESPnet GlobalMVN: (x - mean[m]) * istd[m] on the valid frames, zeros beyond.  grid (ceil(t_max * n_mels / 256), B)
__global__ __launch_bounds__(256) void feat_mvn_kernel(const float* __restrict__ raw, const int32_t* __restrict__ n_frames, int t_max,
                                                       int n_mels, const float* __restrict__ mean, const float* __restrict__ istd,
                                                       float* __restrict__ out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t_max * n_mels) return;
    const int t = i / n_mels, m = i - t * n_mels;
    const size_t at = (size_t)b * t_max * n_mels + i;
    out[at] = t < n_frames[b] ? (raw[at] - mean[m]) * istd[m] : 0.0f;
}

}  // namespace

int rs_launch_frontend(rs_ctx* ctx, const float* audio, const int32_t* lens, int B, int audio_stride,
                       int pad_left, int pad_right, int t_max, float* feats, int32_t* n_frames, float* raw,
                       hipStream_t s) {
    const rs_dims& d = ctx->d;
    if (B <= 0 || t_max <= 0) return RS_OK;
    if (d.n_fft != NFFT) return rs_fail(ctx, RS_EINVAL, "frontend: only n_fft=512 is built");
    if (d.n_mels > 128 || d.n_mels % 4 || d.win_length > NFFT || d.hop_length < 1 || d.hop_length > MAX_HOP)
        return rs_fail(ctx, RS_EINVAL, "frontend: n_mels must be a multiple of 4 up to 128, win <= 512, hop <= %d", MAX_HOP);
    FrontParams p;
    p.audio = audio; p.lens = lens; p.raw = raw; p.n_frames = n_frames;
    p.window = ctx->fe_window; p.twiddle = ctx->fe_twiddle; p.fb_idx = ctx->fe_fb_idx; p.fb_w = ctx->fe_fb_w;
    p.audio_stride = audio_stride; p.pad_left = pad_left; p.pad_right = pad_right; p.t_max = t_max;
    p.n_mels = d.n_mels; p.win_length = d.win_length; p.hop = d.hop_length;
    p.preemph = d.preemph; p.log_guard = d.log_guard;
    p.kind = d.frontend_kind;
    const int fpb = WAVES * FRAMES_PER_WAVE;
    const dim3 grid((t_max + fpb - 1) / fpb, B), block(64 * WAVES);
    if (d.frontend_kind == 2) {                   // kaldi fbank: the log-mel energies ARE the features; frames past an utterance are zeros
        p.raw = feats;
        RS_HIP(ctx, hipMemsetAsync(feats, 0, (size_t)B * t_max * d.n_mels * 4, s));
    }
    const double bytes = (double)B * ((double)t_max * d.hop_length * 4.0 + (double)t_max * d.n_mels * 4.0 * 3.0);
    rs_prof_scope prof(ctx, RS_PROF_FRONTEND, s, (double)B * t_max * (5.0 * 512 * 9 + 3 * 257 + 2 * 600), bytes);
    if (rs_knob(RS_KNOB_LOGMEL_OLD))
        hipLaunchKernelGGL(logmel_kernel<false>, grid, block, 0, s, p);
    else {
        const size_t lds = ((size_t)(fpb - 1) * d.hop_length + NFFT + (size_t)FB_MAXW * (d.n_mels + 1)) * sizeof(float);
        hipLaunchKernelGGL(logmel_kernel<true>, grid, block, lds, s, p);
    }
    if (d.frontend_kind == 2) {
    } else if (d.frontend_kind == 1) {            // (rs_create only: a Conformer context)
        const rs_conformer& cf = *rs_conformer_of(ctx);
        hipLaunchKernelGGL(feat_mvn_kernel, dim3((t_max * d.n_mels + 255) / 256, B), dim3(256), 0, s, raw, n_frames, t_max, d.n_mels,
                           cf.fe_mvn_mean, cf.fe_mvn_istd, feats);
    } else
        hipLaunchKernelGGL(feat_normalize_kernel, dim3(B), dim3(1024), 0, s, raw, n_frames, t_max, d.n_mels, d.norm_eps,
                           feats);
    prof.end();
    RS_CHECK_LAUNCH(ctx, "frontend");
    return RS_OK;
}
