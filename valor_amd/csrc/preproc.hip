// Device-side input preparation: what the reference's AudioMapper / VideoMapper (data/data.py:135-323) compute on the host per clip.
//
// valor_fbank: torchaudio.compliance.kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0) of the SELECTED
//   frames only, normalised and written in the model's [B, A, melbins, T] layout. A block of four waves owns FB_TF = 16 consecutive frames
//   of one output slot (b, a). A wave transforms TWO real frames with ONE complex radix-2 FFT of P points in LDS (frame 0 in the real
//   part, frame 1 in the imaginary part; X0[k] = (Z[k] + conj Z[P-k]) / 2, X1[k] = (Z[k] - conj Z[P-k]) / 2i), then sums the sparse
//   triangular mel filters (rows of consecutive bins, built in fp64 on the host) one filter per lane. The window, the twiddles and the
//   mel weights are host-built tables: no sin / cos is evaluated here. The [melbins][16] tile is staged in LDS so that the stores of
//   the melbins-major output run along T.
//   Arithmetic: fp64 from the sample to the mel energy. Pre-emphasis leaves the lowest filters ~1e-3 of the mean bin power, and the
//   rounding of an fp32 transform is spread evenly over the bins: it costs those filters ~2e-5 in the log, as much as the whole error
//   of an fp32 host filterbank. The transform is a small part of the launch either way, so it is done in the precision that leaves
//   one rounding: the conversion of the energy to fp32 in front of logf.
// valor_frames_prepare: separable bilinear resampling (plain or antialiased, torch.nn.functional.interpolate's two laws) of a crop box
//   of uint8 HWC frames into a window of the virtual resized image, / 255, normalised, optionally mirrored. Coordinates, weights and
//   the accumulation are fp64 (the source index reaches several hundred, where an fp32 fraction keeps only ~15 bits); the pixel values
//   are exact integers, so the one rounding of the result is the final conversion to fp32.
#include "common.h"

#define FB_TF 16                                // frames per block: 4 waves x 2 passes x 2 frames
#define FB_MAX_MEL 256
#define FB_EPS 1.1920929e-07f                   // torch.finfo(torch.float32).eps: the floor of the mel energies
#define FB_LOG_EPS (-15.942385152878742f)       // log(2^-23), rounded to fp32 by the compiler

struct FbankArgs {
    const void* wave; const int64_t* offsets; const int32_t* slice_idx;
    const double* window; const double2* twiddle; const int32_t* mel_start; const int32_t* mel_ptr; const float* mel_w;
    float* out;
    int64_t n_samples;
    int is_pcm16, A, win, shift, P, logP, melbins, T, chunks, mel_nnz;
    float mean, std;
};

DEVINL double fb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVINL double fb_sample(const FbankArgs& a, int64_t i) {
    return (double)(a.is_pcm16 ? (float)((const int16_t*)a.wave)[i] * (1.0f / 32768.0f) : ((const float*)a.wave)[i]);
}

// grid = B * A * ceil(T / 16) blocks of 256 threads; dynamic LDS = 4 * P double2 (one FFT buffer per wave) + melbins * 17 floats
__global__ __launch_bounds__(256) void fbank_kernel(FbankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fb_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double2* Z = (double2*)fb_smem + (size_t)wv * a.P;
    float* stage = (float*)((double2*)fb_smem + (size_t)4 * a.P);             // [melbins][FB_TF + 1]
    const int chunk = blockIdx.x % a.chunks, slot = blockIdx.x / a.chunks;    // slot = b * A + a
    const int b = slot / a.A;
    const int t0 = chunk * FB_TF, nt = min(FB_TF, a.T - t0);
    float* out = a.out + (int64_t)slot * a.melbins * a.T;

    // the clip: samples [lo, lo + N); offsets that leave the buffer make the clip absent instead of a fault
    const int64_t lo = a.offsets[b], hi = a.offsets[b + 1];
    const int sl = a.slice_idx[slot];
    const bool present = sl >= 0 && lo >= 0 && hi >= lo && hi <= a.n_samples;
    const int64_t N = present ? hi - lo : 0;
    const int64_t m = N >= a.win ? 1 + (N - a.win) / a.shift : 0;             // snip_edges framing
    const int64_t f0 = (int64_t)max(sl, 0) * a.T + t0;                        // first frame of this block in the clip's padded fbank
    const float pad_v = (0.0f - a.mean) / (2.0f * a.std);

    if (!present || f0 >= m) {                 // block-uniform: nothing to transform
        const float v = present ? pad_v : 0.0f;
        for (int e = tid; e < a.melbins * nt; e += 256) out[(int64_t)(e / nt) * a.T + t0 + e % nt] = v;
        return;
    }

    for (int pass = 0; pass < 2; ++pass) {
        const int fl = wv * 4 + pass * 2;      // this wave's frame pair inside the block: fl, fl + 1
        const bool r0 = fl < nt && f0 + fl < m, r1 = fl + 1 < nt && f0 + fl + 1 < m;
        const int64_t s0 = lo + (f0 + fl) * a.shift, s1 = s0 + a.shift;
        // frame means
        double sum0 = 0.0, sum1 = 0.0;
        for (int i = lane; i < a.win; i += WAVE) {
            if (r0) sum0 += fb_sample(a, s0 + i);
            if (r1) sum1 += fb_sample(a, s1 + i);
        }
        const double mu0 = fb_wave_sum(sum0) / a.win, mu1 = fb_wave_sum(sum1) / a.win;
        // DC removal, pre-emphasis (x[-1] := x[0]), window, zero padding; stored bit-reversed for the decimation-in-time FFT
        for (int i = lane; i < a.P; i += WAVE) {
            double2 z = {0.0, 0.0};
            if (i < a.win) {
                const int ip = max(i - 1, 0);
                const double w = a.window[i];
                if (r0) z.x = ((fb_sample(a, s0 + i) - mu0) - 0.97 * (fb_sample(a, s0 + ip) - mu0)) * w;
                if (r1) z.y = ((fb_sample(a, s1 + i) - mu1) - 0.97 * (fb_sample(a, s1 + ip) - mu1)) * w;
            }
            Z[__brev((uint32_t)i) >> (32 - a.logP)] = z;
        }
        __syncthreads();
        for (int s = 1; s <= a.logP; ++s) {
            const int half = 1 << (s - 1);
            for (int q = lane; q < a.P / 2; q += WAVE) {
                const int pos = q & (half - 1);
                const int i0 = ((q >> (s - 1)) << s) + pos, i1 = i0 + half;
                const double2 tw = a.twiddle[pos << (a.logP - s)];            // exp(-2 pi i pos / 2^s)
                const double2 u = Z[i0], v = Z[i1];
                const double2 t = {v.x * tw.x - v.y * tw.y, v.x * tw.y + v.y * tw.x};
                Z[i0] = double2{u.x + t.x, u.y + t.y};
                Z[i1] = double2{u.x - t.x, u.y - t.y};
            }
            __syncthreads();
        }
        // power spectra of the two frames, in place: bin k < P/2 reads Z[k] and Z[P - k] (no other lane's bin) and overwrites Z[k]
        for (int k = lane; k < a.P / 2; k += WAVE) {
            const double2 p = Z[k], q = Z[(a.P - k) & (a.P - 1)];
            const double ar = 0.5 * (p.x + q.x), ai = 0.5 * (p.y - q.y);     // X0[k]
            const double br = 0.5 * (p.y + q.y), bi = 0.5 * (q.x - p.x);     // X1[k]
            Z[k] = double2{ar * ar + ai * ai, br * br + bi * bi};
        }
        __syncthreads();
        for (int j = lane; j < a.melbins; j += WAVE) {
            const int st = max(a.mel_start[j], 0), w0 = max(a.mel_ptr[j], 0);
            const int cnt = min(min(a.mel_ptr[j + 1], a.mel_nnz) - w0, a.P / 2 - st);
            double d0 = 0.0, d1 = 0.0;
            for (int t = 0; t < cnt; ++t) {
                const double w = (double)a.mel_w[w0 + t];
                const double2 p = Z[st + t];
                d0 = fma(w, p.x, d0);
                d1 = fma(w, p.y, d1);
            }
            const float e0 = (float)d0, e1 = (float)d1;
            const float l0 = e0 > FB_EPS ? logf(e0) : FB_LOG_EPS, l1 = e1 > FB_EPS ? logf(e1) : FB_LOG_EPS;
            if (fl < nt) stage[j * (FB_TF + 1) + fl] = r0 ? (l0 - a.mean) / (2.0f * a.std) : pad_v;
            if (fl + 1 < nt) stage[j * (FB_TF + 1) + fl + 1] = r1 ? (l1 - a.mean) / (2.0f * a.std) : pad_v;
        }
        __syncthreads();
    }
    // 16 lanes write 16 consecutive floats of one mel row
    for (int e = tid; e < a.melbins * FB_TF; e += 256) {
        const int j = e / FB_TF, t = e % FB_TF;
        if (t < nt) out[(int64_t)j * a.T + t0 + t] = stage[j * (FB_TF + 1) + t];
    }
}

extern "C" int valor_fbank(void* stream, const void* wave, int is_pcm16, int64_t n_samples, const int64_t* offsets, const int32_t* slice_idx,
                           int B, int A, int win, int shift, int P, int melbins, int T, const double* window, const double* twiddle,
                           const int32_t* mel_start, const int32_t* mel_ptr, const float* mel_w, int mel_nnz, float mean, float std,
                           float* out) {
    if (P != 256 && P != 512 && P != 1024 && P != 2048) return VALOR_ERR_ARG;
    if (melbins <= 0 || melbins > FB_MAX_MEL || T <= 0 || win <= P / 2 || win > P || shift <= 0 || mel_nnz <= 0) return VALOR_ERR_ARG;
    if (B < 0 || A <= 0 || n_samples < 0 || !(std != 0.0f)) return VALOR_ERR_ARG;
    if (!offsets || !slice_idx || !window || !twiddle || !mel_start || !mel_ptr || !mel_w || !out || (!wave && n_samples > 0)) return VALOR_ERR_ARG;
    if (B == 0) return VALOR_OK;
    const int64_t chunks = (T + FB_TF - 1) / FB_TF, blocks = (int64_t)B * A * chunks;
    if (blocks > 0x7fffffffll) return VALOR_ERR_ARG;
    FbankArgs a;
    a.wave = wave; a.offsets = offsets; a.slice_idx = slice_idx; a.window = window; a.twiddle = (const double2*)twiddle;
    a.mel_start = mel_start; a.mel_ptr = mel_ptr; a.mel_w = mel_w; a.out = out; a.n_samples = n_samples;
    a.is_pcm16 = is_pcm16 != 0; a.A = A; a.win = win; a.shift = shift; a.P = P; a.logP = __builtin_ctz((unsigned)P); a.melbins = melbins;
    a.T = T; a.chunks = (int)chunks; a.mel_nnz = mel_nnz; a.mean = mean; a.std = std;
    const size_t lds = (size_t)4 * P * sizeof(double2) + (size_t)melbins * (FB_TF + 1) * sizeof(float);
    // P >= 1024: 64 / 128 KiB of FFT buffers + the tile are past the default limit of dynamic LDS (160 KiB per CU: P = 2048 with 256
    // mel bins needs 145 KiB)
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)fbank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return VALOR_ERR_LAUNCH;
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a);
    return valor_launch_status();
}

// ---------------------------------------------------------------- frames
#define FR_GEOM 11       // H, W, top, left, h, w, Hv, Wv, oy, ox, flip

struct FrameArgs {
    const uint8_t* pix; const int64_t* offsets; const int32_t* geom; float* out;
    int64_t n_bytes;
    int R, antialias;
    float mean[3], std[3];
};

// taps [lo, hi) of output index i on an axis of n source pixels, scale = n / n_virtual; weight of tap j by fr_weight
DEVINL void fr_taps(int antialias, double scale, int i, int n, int& lo, int& hi, double& c) {
    if (antialias) {
        const double support = fmax(scale, 1.0);
        c = scale * (i + 0.5);
        lo = max(0, (int)(c - support + 0.5));
        hi = min(n, (int)(c + support + 0.5));
    } else {
        c = fmax(scale * (i + 0.5) - 0.5, 0.0);
        lo = min((int)c, n - 1);
        hi = min(lo + 2, n);
        c -= lo;                                 // lambda (0 where the second tap is clamped away: lo = n - 1)
        if (hi - lo < 2) c = 0.0;
    }
}
DEVINL double fr_weight(int antialias, double scale, double c, int lo, int j) {
    if (antialias) return fmax(0.0, 1.0 - fabs((j - c + 0.5) / fmax(scale, 1.0)));
    return j == lo ? 1.0 - c : c;
}

// grid = F * ceil(R * R / 256): a thread owns output pixel (y, x) of one frame, all three channels
__global__ __launch_bounds__(256) void frames_prepare_kernel(FrameArgs a) {
    const int R = a.R, bpf = (R * R + 255) / 256;
    const int f = blockIdx.x / bpf;
    const int e = (blockIdx.x % bpf) * 256 + threadIdx.x;
    if (e >= R * R) return;
    const int y = e / R, x = e % R;
    const int32_t* g = a.geom + (int64_t)f * FR_GEOM;
    const int H = g[0], W = g[1], top = g[2], left = g[3], h = g[4], w = g[5], Hv = g[6], Wv = g[7], oy = g[8], ox = g[9], flip = g[10];
    float* out = a.out + (int64_t)f * 3 * R * R + (int64_t)y * R + x;
    const int64_t off = a.offsets[f];
    // a row that does not describe pixels inside the buffer reads nothing: the frame becomes NaN
    const bool ok = H > 0 && W > 0 && h > 0 && w > 0 && top >= 0 && left >= 0 && (int64_t)top + h <= H && (int64_t)left + w <= W && Hv > 0 && Wv > 0 &&
                    oy >= 0 && ox >= 0 && (int64_t)oy + R <= Hv && (int64_t)ox + R <= Wv && off >= 0 && off + (int64_t)H * W * 3 <= a.n_bytes;
    if (!ok) {
        for (int c = 0; c < 3; ++c) out[(int64_t)c * R * R] = __builtin_nanf("");
        return;
    }
    const double sy = (double)h / Hv, sx = (double)w / Wv;
    int ylo, yhi, xlo, xhi;
    double cy, cx;
    fr_taps(a.antialias, sy, y + oy, h, ylo, yhi, cy);
    fr_taps(a.antialias, sx, (flip ? R - 1 - x : x) + ox, w, xlo, xhi, cx);
    const uint8_t* src = a.pix + off;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wys = 0.0, wxs = 0.0;
    for (int j = xlo; j < xhi; ++j) wxs += fr_weight(a.antialias, sx, cx, xlo, j);
    for (int i = ylo; i < yhi; ++i) {
        const double wy = fr_weight(a.antialias, sy, cy, ylo, i);
        wys += wy;
        const uint8_t* row = src + ((int64_t)(top + i) * W + left) * 3;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int j = xlo; j < xhi; ++j) {
            const double wx = fr_weight(a.antialias, sx, cx, xlo, j);
            r0 = fma(wx, (double)row[j * 3 + 0], r0);
            r1 = fma(wx, (double)row[j * 3 + 1], r1);
            r2 = fma(wx, (double)row[j * 3 + 2], r2);
        }
        acc0 = fma(wy, r0, acc0);
        acc1 = fma(wy, r1, acc1);
        acc2 = fma(wy, r2, acc2);
    }
    const double inv = 1.0 / (wys * wxs * 255.0);
    out[0] = (float)((acc0 * inv - (double)a.mean[0]) / (double)a.std[0]);
    out[(int64_t)R * R] = (float)((acc1 * inv - (double)a.mean[1]) / (double)a.std[1]);
    out[(int64_t)2 * R * R] = (float)((acc2 * inv - (double)a.mean[2]) / (double)a.std[2]);
}

extern "C" int valor_frames_prepare(void* stream, const uint8_t* pixels, int64_t n_bytes, const int64_t* offsets, const int32_t* geom, int F,
                                    int R, int antialias, const float* mean, const float* std, float* out) {
    if (R <= 0 || R > 4096 || F < 0 || n_bytes < 0) return VALOR_ERR_ARG;
    if (!offsets || !geom || !mean || !std || !out || (!pixels && n_bytes > 0)) return VALOR_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!(std[c] != 0.0f)) return VALOR_ERR_ARG;
    if (F == 0) return VALOR_OK;
    const int64_t blocks = (int64_t)F * ((R * R + 255) / 256);
    if (blocks > 0x7fffffffll) return VALOR_ERR_ARG;
    FrameArgs a;
    a.pix = pixels; a.offsets = offsets; a.geom = geom; a.out = out; a.n_bytes = n_bytes; a.R = R; a.antialias = antialias != 0;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
    hipLaunchKernelGGL(frames_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return valor_launch_status();
}
