// Audio front end: framing -> Hann -> real FFT -> |.|^2 -> sparse Slaney mel -> log (or dB, or power -> PCEN).
// logmel_kernel is the 512-point kernel of the build-defined configuration; logmel_ex_kernel (further down) serves
// n_fft 256-2048, up to 128 bands and the dB and power scales.  Both have a stream form (logmel_stream_kernel,
// logmel_ex_stream_kernel) for ONE long recording: the grid runs over runs of its frames instead of over clips, the frame
// arithmetic is the same __device__ function.
// North-star addition beneath the reference's data loader (the reference ships
// pre-extracted features only: nsga_penalty.py:64-71); the
// algorithm restates librosa.feature.melspectrogram (requirements.txt:80) and is
// checked against oracle/frontend.py.
//
// One 256-thread workgroup per clip, each wave owns one frame at a time.  A frame is one
// coalesced 2 KB segment of the clip; the 3.2x overlap between consecutive frames is served
// by L2, so HBM sees each clip once (64 000 B in, T*n_mels*4 B out).
// The 512 real samples are packed into 256 complex points (even + i*odd) and transformed by a
// 256-point radix-4 decimation-in-frequency FFT held in registers: each lane owns one radix-4
// butterfly per stage (4 stages), with three exchanges through the wave's own LDS scratch
// (padded so every ds_read/write_b64 is conflict-free) and every twiddle / window value
// precomputed per lane in registers outside the frame loop.  The real-FFT split
// X[k] = E[k] + W^k O[k] follows in LDS-skewed natural order, then the sparse mel: each band is one
// lane's short loop, the widest bands split over two lanes, summed in fixed order.
// Only wave-level synchronisation (LDS operations of one wave complete in issue order).
// Measured 2.19 ms for 30 000 one-second clips = 1.10 TB/s of algorithmic bytes (13.7 % of the HBM roofline;
// the 15 kFLOP of fp32 VALU work per 792-byte frame, not HBM, bounds it); the radix-2 LDS FFT it replaces took 10.3 ms.
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace cmoop {

struct FrontendTables {
    FrontendCfg cfg;
    bool general = false;      // tables of logmel_ex_kernel (below) instead of logmel_kernel's
    float* tw = nullptr;       // logmel_kernel: [n_fft/2][2] cos, -sin ; general: the whole circle, [n_fft][2]
    float* win = nullptr;      // [n_fft] padded periodic Hann
    float* melw = nullptr;     // sparse weights, band after band
    int* meltask = nullptr;    // logmel_kernel: [64][3] first bin, count, weight offset of each lane's task ; then [64] second task of a band or -1
                               // general: [n_mels][3] first bin, count, weight offset of each band
    int nnz = 0;
};

static double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

bool frontend_cfg_equal(const FrontendCfg& a, const FrontendCfg& b) {
    return a.sr == b.sr && a.n_fft == b.n_fft && a.win == b.win && a.hop == b.hop && a.n_mels == b.n_mels && a.fmin == b.fmin &&
           a.fmax == b.fmax && a.log_eps == b.log_eps && a.scale == b.scale && a.db_ref_max == b.db_ref_max &&
           a.db_amin == b.db_amin && a.top_db == b.top_db;
}

bool frontend_uses_fixed_kernel(const FrontendCfg& c) { return c.n_fft == 512 && c.n_mels <= 64 && c.scale == 0; }

void frontend_check(const FrontendCfg& c) {
    auto fail = [](const char* field, const std::string& rule) { throw std::runtime_error(std::string("front end config: ") + field + " " + rule); };
    if (c.sr <= 0) fail("sr", "must be positive (got " + std::to_string(c.sr) + ")");
    if (c.n_fft != 256 && c.n_fft != 512 && c.n_fft != 1024 && c.n_fft != 2048)
        fail("n_fft", "must be 256, 512, 1024 or 2048 (got " + std::to_string(c.n_fft) + ")");
    if (c.win < 1 || c.win > c.n_fft) fail("win", "must lie in 1..n_fft (got " + std::to_string(c.win) + ")");
    if (c.hop < 1) fail("hop", "must be at least 1 (got " + std::to_string(c.hop) + ")");
    if (c.n_mels < 1 || c.n_mels > FRONTEND_MAX_MELS) fail("n_mels", "must lie in 1..128 (got " + std::to_string(c.n_mels) + ")");
    if (!(c.fmax <= 0.5f * (float)c.sr)) fail("fmax", "must not exceed sr/2 (got " + std::to_string(c.fmax) + ")");
    if (!(c.fmin >= 0.f && c.fmin < c.fmax)) fail("fmin", "must satisfy 0 <= fmin < fmax (got " + std::to_string(c.fmin) + ")");
    if (c.scale != 0 && c.scale != 1 && c.scale != 2) fail("scale", "must be 0 (log), 1 (dB) or 2 (power)");
    if (c.scale == 0 && !(c.log_eps > 0.f)) fail("log_eps", "must be positive");
    if (c.scale == 1 && !(c.db_amin > 0.f)) fail("db_amin", "must be positive");
    if (c.scale == 1 && !(c.top_db == c.top_db)) fail("top_db", "must be a number (negative: no clip)");
}

// Host-side tables in double, stored as float: twiddles exp(-2 pi i k / n_fft) for the whole circle, the periodic Hann
// of win points centred in n_fft, and the Slaney mel basis (librosa.filters.mel, norm='slaney') as one run of
// consecutive non-zero weights per band.  Nothing here touches the GPU.
FrontendHostTables frontend_host_tables(const FrontendCfg& c) {
    frontend_check(c);
    FrontendHostTables h;
    const int half = c.n_fft / 2, nb = half + 1;
    h.tw.resize(2 * c.n_fft);
    h.win.assign(c.n_fft, 0.f);
    for (int k = 0; k < c.n_fft; ++k) {
        const double a = -2.0 * M_PI * k / c.n_fft;
        h.tw[2 * k] = (float)std::cos(a);
        h.tw[2 * k + 1] = (float)std::sin(a);
    }
    const int lpad = (c.n_fft - c.win) / 2;
    for (int n = 0; n < c.win; ++n) h.win[lpad + n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c.win));
    std::vector<double> mel_f(c.n_mels + 2);
    const double m_lo = hz_to_mel(c.fmin), m_hi = hz_to_mel(c.fmax);
    for (int i = 0; i < c.n_mels + 2; ++i) mel_f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (c.n_mels + 1));
    h.first_bin.resize(c.n_mels); h.count.resize(c.n_mels); h.start.resize(c.n_mels);
    for (int i = 0; i < c.n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        int first = -1, cnt = 0;
        h.start[i] = (int)h.melw.size();
        for (int b = 0; b < nb; ++b) {
            const double f = (double)b * (c.sr / 2.0) / half;
            const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
            const double v = std::max(0.0, std::min(lower, upper)) * enorm;
            if (v > 0.0) {
                if (first < 0) first = b;
                CMOOP_REQUIRE(b == first + cnt, "front end: a mel band's bins are not contiguous");
                h.melw.push_back((float)v);     // bins of one triangle are contiguous
                ++cnt;
            }
        }
        h.first_bin[i] = first < 0 ? 0 : first;
        h.count[i] = cnt;
    }
    // a bin lies strictly inside at most two triangles
    CMOOP_REQUIRE((int)h.melw.size() <= 2 * nb, "front end: mel table too large");
    return h;
}

FrontendTables* frontend_tables_create(const FrontendCfg& c) {
    const FrontendHostTables h = frontend_host_tables(c);
    auto* t = new FrontendTables;
    t->cfg = c;
    t->general = !frontend_uses_fixed_kernel(c);
    const int half = c.n_fft / 2;
    std::vector<float> tw(h.tw.begin(), h.tw.begin() + 2 * (t->general ? c.n_fft : half));
    std::vector<float> w = h.melw;
    std::vector<int> task;
    if (t->general) {
        task.resize(3 * c.n_mels);
        for (int i = 0; i < c.n_mels; ++i) { task[3 * i] = h.first_bin[i]; task[3 * i + 1] = h.count[i]; task[3 * i + 2] = h.start[i]; }
    } else {
        // lane tasks: task i < n_mels = band i; the spare lanes take the second half of the widest bands
        const std::vector<int>&first_bin = h.first_bin, &count = h.count, &start = h.start;
        task.assign(64 * 3 + 64, 0);
        for (int i = 0; i < 64; ++i) task[192 + i] = -1;
        for (int i = 0; i < c.n_mels; ++i) { task[3 * i] = first_bin[i]; task[3 * i + 1] = count[i]; task[3 * i + 2] = start[i]; }
        std::vector<int> order(c.n_mels);
        for (int i = 0; i < c.n_mels; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count[a] > count[b]; });
        int next = c.n_mels;
        for (int oi = 0; oi < c.n_mels && next < 64; ++oi) {
            const int b = order[oi];
            if (count[b] < 8) break;
            const int hh = count[b] / 2;                 // first task keeps bins [0, hh), second [hh, count)
            task[3 * b + 1] = hh;
            task[3 * next] = first_bin[b] + hh; task[3 * next + 1] = count[b] - hh; task[3 * next + 2] = start[b] + hh;
            task[192 + b] = next;
            ++next;
        }
        CMOOP_REQUIRE(w.size() <= 1024, "front end: mel table too large");
    }
    t->nnz = (int)w.size();
    if (w.empty()) w.push_back(0.f);
    try {
        CMOOP_HIP(hipMalloc(&t->tw, tw.size() * 4));
        CMOOP_HIP(hipMalloc(&t->win, h.win.size() * 4));
        CMOOP_HIP(hipMalloc(&t->melw, w.size() * 4));
        CMOOP_HIP(hipMalloc(&t->meltask, task.size() * 4));
        CMOOP_HIP(hipMemcpy(t->tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
        CMOOP_HIP(hipMemcpy(t->win, h.win.data(), h.win.size() * 4, hipMemcpyHostToDevice));
        CMOOP_HIP(hipMemcpy(t->melw, w.data(), w.size() * 4, hipMemcpyHostToDevice));
        CMOOP_HIP(hipMemcpy(t->meltask, task.data(), task.size() * 4, hipMemcpyHostToDevice));
    } catch (...) {
        frontend_tables_destroy(t);
        throw;
    }
    return t;
}

void frontend_tables_destroy(FrontendTables* t) {
    if (!t) return;
    hipFree(t->tw); hipFree(t->win); hipFree(t->melw); hipFree(t->meltask);
    delete t;
}

constexpr int NFFT = 512, NC = 256;   // real points, packed complex points

// Each wave owns its scratch, so the phases only need the wave's own LDS writes to be visible to its
// other lanes: LDS operations of one wave complete in issue order; the fences only stop the compiler
// from moving the reads above the writes.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ f32x2 cmul(const f32x2 a, const f32x2 w) {
    return f32x2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x};
}
// radix-4 forward butterfly: b_j = sum_p a_p (-i)^(p j)
__device__ __forceinline__ void bfly4(const f32x2 a0, const f32x2 a1, const f32x2 a2, const f32x2 a3, f32x2& b0, f32x2& b1,
                                      f32x2& b2, f32x2& b3) {
    const f32x2 s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = a1 - a3;
    const f32x2 nid = f32x2{d13.y, -d13.x};   // -i * d13
    b0 = s02 + s13;
    b2 = s02 - s13;
    b1 = d02 + nid;
    b3 = d02 - nid;
}

// Frames [f0, f1) of one waveform `clip`, written to rows f0.. of `rows` ([.][n_mels]): the whole per-frame arithmetic
// of the 512-point kernel.  logmel_kernel runs it over a clip's frames, logmel_stream_kernel over one run of a recording's.
__device__ __forceinline__ void logmel_frames(const float* __restrict__ clip, int n_samples, float* __restrict__ rows,
                                              int f0, int f1, int hop, int n_mels, float log_eps,
                                              const float* __restrict__ g_tw, const float* __restrict__ g_win,
                                              const float* __restrict__ g_melw, const int* __restrict__ g_task,
                                              int nnz) {
    constexpr int XB = 320;    // complex slots of the exchange buffer (pitch-20 / pitch-5 layouts, skewed spectrum)
    constexpr int PB = 264;    // power spectrum bins 0..256
    __shared__ float s_melw[1024];
    __shared__ int s_task[256];
    __shared__ __attribute__((aligned(16))) f32x2 s_x[4][XB];
    __shared__ float s_p[4][PB];
    __shared__ float s_part[4][64];

    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = t; i < nnz; i += 256) s_melw[i] = g_melw[i];
    s_task[t] = g_task[t];
    __syncthreads();

    // ---- per-lane constants, fixed over the frames -------------------------------------------------
    const f32x2* tw = reinterpret_cast<const f32x2*>(g_tw);   // tw[k] = exp(-2 pi i k / 512), k < 256
    auto tw512 = [&](int k) {                                 // k < 512: W^(k + 256) = -W^k
        const f32x2 v = tw[k & 255];
        return (k & 256) ? -v : v;
    };
    f32x2 w0[3], w1[3], w2[3], wp[4];
    float win[8];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        w0[j - 1] = tw512(2 * ((lane * j) & 255));           // W_256^(l j)
        w1[j - 1] = tw512(8 * (((lane & 15) * j) & 63));     // W_64^(n j),  n = l & 15
        w2[j - 1] = tw512(32 * (((lane & 3) * j) & 15));     // W_16^(n j),  n = l & 3
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        wp[u] = tw[lane + 64 * u];                            // W_512^k, k = lane + 64 u
        win[2 * u] = g_win[2 * (lane + 64 * u)];
        win[2 * u + 1] = g_win[2 * (lane + 64 * u) + 1];
    }
    const int j1 = lane >> 4, n1 = lane & 15;                 // stage 1: sub-FFT j1 of 64 points, butterfly n1
    const int s2 = lane >> 2, n2 = lane & 3;                  // stage 2: sub-FFT s2 of 16 points, butterfly n2
    const int klow = (lane >> 4) + 4 * ((lane >> 2) & 3) + 16 * (lane & 3);   // stage 3: output bins klow + 64 j4
    const int task_first = s_task[3 * lane], task_cnt = s_task[3 * lane + 1], task_w = s_task[3 * lane + 2];
    const int task2 = s_task[192 + lane];

    f32x2* xb = s_x[wave];
    float* pw = s_p[wave];
    float* part = s_part[wave];
    for (int frame = f0 + wave; frame < f1; frame += 4) {     // wave-uniform; no workgroup barrier below
        // windowed frame, centre-padded with zeros (pad_mode='constant'); z[m] = x[2m] + i x[2m+1]
        const int base = frame * hop - NFFT / 2;
        f32x2 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i0 = base + 2 * (lane + 64 * u);
            const float x0 = (i0 >= 0 && i0 < n_samples) ? clip[i0] : 0.f;
            const float x1 = (i0 + 1 >= 0 && i0 + 1 < n_samples) ? clip[i0 + 1] : 0.f;
            a[u] = f32x2{x0 * win[2 * u], x1 * win[2 * u + 1]};
        }
        // stage 0: points l + 64 p  ->  four 64-point sequences y_j[l]
        bfly4(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
        xb[lane] = b[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) xb[64 * j + lane] = cmul(b[j], w0[j - 1]);
        wave_sync();
        // stage 1: y_j[n + 16 p] -> sixteen 16-point sequences, stored with pitch 20
#pragma unroll
        for (int p = 0; p < 4; ++p) a[p] = xb[64 * j1 + n1 + 16 * p];
        wave_sync();
        bfly4(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
        xb[(4 * j1) * 20 + n1] = b[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) xb[(4 * j1 + j) * 20 + n1] = cmul(b[j], w1[j - 1]);
        wave_sync();
        // stage 2: u[n + 4 p] -> sixty-four 4-point sequences, stored with pitch 5
#pragma unroll
        for (int p = 0; p < 4; ++p) a[p] = xb[20 * s2 + n2 + 4 * p];
        wave_sync();
        bfly4(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
        xb[(4 * s2) * 5 + n2] = b[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) xb[(4 * s2 + j) * 5 + n2] = cmul(b[j], w2[j - 1]);
        wave_sync();
        // stage 3: 4-point transforms; Z[k], k = klow + 64 j4, stored in natural order skewed by k >> 4
#pragma unroll
        for (int p = 0; p < 4; ++p) a[p] = xb[5 * lane + p];
        wave_sync();
        bfly4(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = klow + 64 * j;
            xb[k + (k >> 4)] = b[j];
        }
        wave_sync();
        // real-FFT split and power spectrum: X[k] = E[k] + W_512^k O[k], E = (Z[k] + conj Z[256-k]) / 2, O = (Z[k] - conj Z[256-k]) / 2i
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = lane + 64 * u, kc = (NC - k) & (NC - 1);
            const f32x2 z = xb[k + (k >> 4)], zc = xb[kc + (kc >> 4)];
            const f32x2 e = f32x2{0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y)};
            const f32x2 o = f32x2{0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x)};
            const f32x2 x = e + cmul(o, wp[u]);
            pw[k] = x.x * x.x + x.y * x.y;
            if (k == 0) {                                     // bin 256: E[0] - O[0]
                const float xn = e.x - o.x;
                pw[NC] = xn * xn;
            }
        }
        wave_sync();
        // sparse mel: one short loop per lane task, second halves of the widest bands on the spare lanes
        {
            float acc = 0.f;
            for (int i = 0; i < task_cnt; ++i) acc = fmaf(s_melw[task_w + i], pw[task_first + i], acc);
            part[lane] = acc;
        }
        wave_sync();
        if (lane < n_mels) {
            float acc = part[lane];
            if (task2 >= 0) acc += part[task2];
            rows[(size_t)frame * n_mels + lane] = logf(acc + log_eps);
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wav, int n_samples, float* __restrict__ out,
                                                     int T, int hop, int n_mels, float log_eps,
                                                     const float* __restrict__ g_tw, const float* __restrict__ g_win,
                                                     const float* __restrict__ g_melw, const int* __restrict__ g_task,
                                                     int nnz) {
    logmel_frames(wav + (size_t)blockIdx.x * n_samples, n_samples, out + (size_t)blockIdx.x * T * n_mels, 0, T, hop, n_mels,
                  log_eps, g_tw, g_win, g_melw, g_task, nnz);
}

// Stream form: ONE recording, workgroup b owns frames [b run, min((b + 1) run, T)) -- a wave still owns a frame at a time,
// so frame f carries the bits logmel_kernel gives it.  Every workgroup re-loads the tables (the prologue of logmel_frames).
__global__ __launch_bounds__(256) void logmel_stream_kernel(const float* __restrict__ wav, int n_samples, float* __restrict__ out,
                                                            int T, int run, int hop, int n_mels, float log_eps,
                                                            const float* __restrict__ g_tw, const float* __restrict__ g_win,
                                                            const float* __restrict__ g_melw, const int* __restrict__ g_task,
                                                            int nnz) {
    const int f0 = blockIdx.x * run;                          // < T: the grid is ceil(T / run)
    logmel_frames(wav, n_samples, out, f0, f0 + min(run, T - f0), hop, n_mels, log_eps, g_tw, g_win, g_melw, g_task, nnz);
}

// ---- general geometry: n_fft 256 / 512 / 1024 / 2048, up to 128 mel bands, log or dB scale ---------------------------
// Same shape as logmel_kernel (one workgroup per clip, a wave owns a frame at a time, wave-level synchronisation only),
// but the packed NC = n_fft/2 complex points live in the wave's own LDS buffer instead of registers: a lane would hold up
// to 16 points.  The transform is a Stockham radix-4 decimation-in-time FFT with a radix-2 tail where log2 NC is odd
// (NC 128, 512): stage Ns (1, 4, 16, ...) reads points j + r NC/4, multiplies by W_(4Ns)^(r (j mod Ns)), and stores
// the butterfly at (j / Ns) 4 Ns + (j mod Ns) + r Ns, so input and output are both in natural order.  Every lane reads
// all its points of a stage into registers before any lane stores, which makes the exchange in place (8 KiB per wave at
// n_fft 2048).  Loads of a stage are consecutive complex points across lanes; the stores of the first two stages are not
// (pitch 4 and 16), so slot i is kept at ex_slot(i), a rotation inside each aligned run of 16 points by 5 (i / 16):
// loads stay conflict-free (an aligned run of 32 points still fills 32 distinct 8-byte slots), the pitch-4 stores become
// conflict-free and the pitch-16 stores two-way; later stages store runs of >= 16 consecutive points.
// Twiddles, window and the real-split factors are per-lane registers, read once from the host-built double tables.
// The mel bands are lane i & 63, bands 0-63 first and then 64-127, each a serial loop in bin order (deterministic).
// dB scale: the workgroup stores 10 log10(max(amin, S)), reduces the clip's maximum over its waves, barriers, then
// subtracts the reference and applies the top_db floor to its own rows -- no second launch, no atomics.
__device__ __forceinline__ int ex_slot(const int i) { return (i & ~15) | ((i + 5 * (i >> 4)) & 15); }

// Frames [f0, f1) of one waveform `clip`, written to rows f0.. of `rows` ([.][n_mels]) as log(mel + eps), as the
// un-referenced 10 log10(max(amin, mel)) or as the mel power itself (scale 2); returns this lane's largest stored value
// (dB scale).  Shared by logmel_ex_kernel (a clip's frames, then the dB tail), logmel_pcen_kernel (a clip's frames, then
// the PCEN recurrence) and logmel_ex_stream_kernel (one run of a recording's frames).
template <int NC>
__device__ __forceinline__ float logmel_ex_frames(const float* __restrict__ clip, int n_samples, float* __restrict__ rows,
                                                  int f0, int f1, int hop, int n_mels, int scale, float log_eps, float amin,
                                                  const float* __restrict__ g_tw, const float* __restrict__ g_win,
                                                  const float* __restrict__ g_melw, const int* __restrict__ g_band, int nnz) {
    constexpr int LG = NC == 128 ? 7 : NC == 256 ? 8 : NC == 512 ? 9 : 10;
    constexpr int S4 = LG / 2;                                   // radix-4 stages
    constexpr bool TAIL2 = (LG & 1) != 0;
    constexpr int B4 = NC >= 256 ? NC / 256 : 1;                 // radix-4 butterflies per lane (NC 128: lanes 0-31 only)
    constexpr int B2 = NC / 128;                                 // radix-2 butterflies per lane in the tail
    constexpr int U = NC / 64;                                   // spectrum bins per lane in the real split
    __shared__ float s_melw[2 * (NC + 1)];
    __shared__ __attribute__((aligned(16))) f32x2 s_x[4][NC];
    __shared__ float s_p[4][NC + 4];

    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = t; i < nnz; i += 256) s_melw[i] = g_melw[i];
    __syncthreads();

    // ---- per-lane constants, fixed over the frames -------------------------------------------------
    const f32x2* tw = reinterpret_cast<const f32x2*>(g_tw);      // tw[k] = exp(-2 pi i k / n_fft), k < n_fft = 2 NC
    f32x2 w4[S4 > 1 ? S4 - 1 : 1][B4][3], w2[TAIL2 ? B2 : 1], wp[U];
    float win[B4][4][2];
#pragma unroll
    for (int b = 0; b < B4; ++b) {
        const int j = lane + 64 * b;
        const bool on = j < NC / 4;
#pragma unroll
        for (int st = 1; st < S4; ++st) {
            const int k = j & ((1 << (2 * st)) - 1);             // j mod Ns, Ns = 4^st
#pragma unroll
            for (int r = 1; r < 4; ++r) w4[st - 1][b][r - 1] = tw[on ? (k * r) << (LG - 1 - 2 * st) : 0];   // W_(4Ns)^(k r)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = on ? j + r * (NC / 4) : 0;
            win[b][r][0] = g_win[2 * m];
            win[b][r][1] = g_win[2 * m + 1];
        }
    }
    if (TAIL2) {
#pragma unroll
        for (int b = 0; b < B2; ++b) w2[b] = tw[2 * (lane + 64 * b)];     // W_NC^j, j < NC/2
    }
#pragma unroll
    for (int u = 0; u < U; ++u) wp[u] = tw[lane + 64 * u];               // W_nfft^k
    int band_first[2], band_cnt[2], band_w[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int band = lane + 64 * h;
        const bool on = band < n_mels;
        band_first[h] = on ? g_band[3 * band] : 0;
        band_cnt[h] = on ? g_band[3 * band + 1] : 0;
        band_w[h] = on ? g_band[3 * band + 2] : 0;
    }

    f32x2* xb = s_x[wave];
    float* pw = s_p[wave];
    float vmax = -INFINITY;                                      // dB scale: this lane's largest stored value
    for (int frame = f0 + wave; frame < f1; frame += 4) {        // wave-uniform; no workgroup barrier inside the loop
        const int base = frame * hop - NC;                       // centre padding: n_fft / 2 zeros on either side
        f32x2 a[B4][4], v[4];
        // stage 0 (Ns = 1, no twiddles) straight from the windowed frame: z[m] = x[2m] + i x[2m+1]
#pragma unroll
        for (int b = 0; b < B4; ++b) {
            const int j = lane + 64 * b;
            if (j < NC / 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i0 = base + 2 * (j + r * (NC / 4));
                    const float x0 = (i0 >= 0 && i0 < n_samples) ? clip[i0] : 0.f;
                    const float x1 = (i0 + 1 >= 0 && i0 + 1 < n_samples) ? clip[i0 + 1] : 0.f;
                    a[b][r] = f32x2{x0 * win[b][r][0], x1 * win[b][r][1]};
                }
                bfly4(a[b][0], a[b][1], a[b][2], a[b][3], v[0], v[1], v[2], v[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r) xb[ex_slot(4 * j + r)] = v[r];
            }
        }
        wave_sync();
#pragma unroll
        for (int st = 1; st < S4; ++st) {
            const int ns = 1 << (2 * st);
#pragma unroll
            for (int b = 0; b < B4; ++b) {
                const int j = lane + 64 * b;
                if (j < NC / 4) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[b][r] = xb[ex_slot(j + r * (NC / 4))];
                }
            }
            wave_sync();
#pragma unroll
            for (int b = 0; b < B4; ++b) {
                const int j = lane + 64 * b;
                if (j < NC / 4) {
                    bfly4(a[b][0], cmul(a[b][1], w4[st - 1][b][0]), cmul(a[b][2], w4[st - 1][b][1]), cmul(a[b][3], w4[st - 1][b][2]),
                          v[0], v[1], v[2], v[3]);
                    const int d = ((j >> (2 * st)) << (2 * st + 2)) + (j & (ns - 1));
#pragma unroll
                    for (int r = 0; r < 4; ++r) xb[ex_slot(d + r * ns)] = v[r];
                }
            }
            wave_sync();
        }
        if (TAIL2) {
            f32x2 p0[B2], p1[B2];
#pragma unroll
            for (int b = 0; b < B2; ++b) {
                const int j = lane + 64 * b;
                p0[b] = xb[ex_slot(j)];
                p1[b] = xb[ex_slot(j + NC / 2)];
            }
            wave_sync();
#pragma unroll
            for (int b = 0; b < B2; ++b) {
                const int j = lane + 64 * b;
                const f32x2 q = cmul(p1[b], w2[b]);
                xb[ex_slot(j)] = p0[b] + q;
                xb[ex_slot(j + NC / 2)] = p0[b] - q;
            }
            wave_sync();
        }
        // real-FFT split and power spectrum: X[k] = E[k] + W_nfft^k O[k], E = (Z[k] + conj Z[NC-k]) / 2, O = (Z[k] - conj Z[NC-k]) / 2i
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = lane + 64 * u, kc = (NC - k) & (NC - 1);
            const f32x2 z = xb[ex_slot(k)], zc = xb[ex_slot(kc)];
            const f32x2 e = f32x2{0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y)};
            const f32x2 o = f32x2{0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x)};
            const f32x2 x = e + cmul(o, wp[u]);
            pw[k] = x.x * x.x + x.y * x.y;
            if (k == 0) {                                        // bin NC: E[0] - O[0]
                const float xn = e.x - o.x;
                pw[NC] = xn * xn;
            }
        }
        wave_sync();
        // sparse mel: band lane + 64 h, bins in ascending order; a band without a bin stores log(eps) / the amin floor
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int band = lane + 64 * h;
            float acc = 0.f;
            for (int i = 0; i < band_cnt[h]; ++i) acc = fmaf(s_melw[band_w[h] + i], pw[band_first[h] + i], acc);
            if (band < n_mels) {
                float y;
                if (scale == 0) {
                    y = logf(acc + log_eps);
                } else if (scale == 1) {
                    y = 10.f * log10f(fmaxf(amin, acc));
                    vmax = fmaxf(vmax, y);
                } else {
                    y = acc;                                     // linear mel power; a band without a bin stores 0
                }
                rows[(size_t)frame * n_mels + band] = y;
            }
        }
        wave_sync();
    }
    return vmax;
}

template <int NC>
__global__ __launch_bounds__(256) void logmel_ex_kernel(const float* __restrict__ wav, int n_samples, float* __restrict__ out,
                                                        int T, int hop, int n_mels, int scale, int db_ref_max, float log_eps,
                                                        float amin, float top_db, const float* __restrict__ g_tw,
                                                        const float* __restrict__ g_win, const float* __restrict__ g_melw,
                                                        const int* __restrict__ g_band, int nnz) {
    __shared__ float s_red[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    float* rows = out + (size_t)blockIdx.x * T * n_mels;
    float vmax = logmel_ex_frames<NC>(wav + (size_t)blockIdx.x * n_samples, n_samples, rows, 0, T, hop, n_mels, scale, log_eps,
                                      amin, g_tw, g_win, g_melw, g_band, nnz);
    if (scale != 1) return;                                      // kernel argument: uniform over the grid
    // dB scale: reference and top_db floor from the clip's own maximum, applied to the rows this workgroup stored
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
    if (lane == 0) s_red[wave] = vmax;
    __syncthreads();                                             // also orders the waves' stores to out before the reads below
    const float cmax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    const float ref = db_ref_max ? cmax : 10.f * log10f(fmaxf(amin, 1.f));
    const float floor_db = top_db >= 0.f ? (cmax - ref) - top_db : -INFINITY;
    const int total = T * n_mels;
    for (int i = t; i < total; i += 256) rows[i] = fmaxf(rows[i] - ref, floor_db);
}

// Stream form of the general kernel: ONE recording, workgroup b owns frames [b run, min((b + 1) run, T)).  No dB tail:
// a recording has no clip maximum; the reference and the top_db floor belong to the windows cut from the stream later
// (window_gather_kernel, augment.hip), so the dB scale leaves the un-referenced 10 log10(max(amin, mel)) here.
template <int NC>
__global__ __launch_bounds__(256) void logmel_ex_stream_kernel(const float* __restrict__ wav, int n_samples, float* __restrict__ out,
                                                               int T, int run, int hop, int n_mels, int scale, float log_eps,
                                                               float amin, const float* __restrict__ g_tw,
                                                               const float* __restrict__ g_win, const float* __restrict__ g_melw,
                                                               const int* __restrict__ g_band, int nnz) {
    const int f0 = blockIdx.x * run;                             // < T: the grid is ceil(T / run)
    logmel_ex_frames<NC>(wav, n_samples, out, f0, f0 + min(run, T - f0), hop, n_mels, scale, log_eps, amin, g_tw, g_win, g_melw,
                         g_band, nnz);
}

// The general kernels exist for the four FFT sizes: f(std::integral_constant<int, n_fft / 2>()) hands the launcher its
// packed complex point count as a compile-time constant (the kernels' template argument)
template <class F>
static void with_fft_points(int n_fft, F&& f) {
    if (n_fft == 256) f(std::integral_constant<int, 128>());
    else if (n_fft == 512) f(std::integral_constant<int, 256>());
    else if (n_fft == 1024) f(std::integral_constant<int, 512>());
    else f(std::integral_constant<int, 1024>());
}

int frontend_frames(const FrontendCfg& c, int n_samples) {
    CMOOP_REQUIRE(n_samples >= 1, "front end: n_samples must be at least 1");
    CMOOP_REQUIRE(c.hop >= 1, "front end config: hop must be at least 1");
    const int64_t T = 1 + (int64_t)n_samples / c.hop;
    CMOOP_REQUIRE(T <= 0x7fffffff, "front end: too many frames");
    return (int)T;
}

void launch_logmel(const float* wav, int64_t n_clips, int n_samples, float* out, const FrontendTables* t, hipStream_t s) {
    const FrontendCfg& c = t->cfg;
    const int T = frontend_frames(c, n_samples);
    CMOOP_REQUIRE(n_clips >= 0 && n_clips <= 0x7fffffff && (int64_t)T * c.n_mels <= 0x7fffffff, "front end: clip count / clip length out of range");
    if (n_clips == 0) return;
    CMOOP_REQUIRE(wav && out, "front end: NULL buffer");
    if (!t->general) {
        hipLaunchKernelGGL(logmel_kernel, dim3((unsigned)n_clips), dim3(256), 0, s, wav, n_samples, out, T, c.hop, c.n_mels,
                           c.log_eps, t->tw, t->win, t->melw, t->meltask, t->nnz);
    } else {
        with_fft_points(c.n_fft, [&](auto nc) {
            hipLaunchKernelGGL(logmel_ex_kernel<decltype(nc)::value>, dim3((unsigned)n_clips), dim3(256), 0, s, wav, n_samples, out, T,
                               c.hop, c.n_mels, c.scale, c.db_ref_max, c.log_eps, c.db_amin, c.top_db, t->tw, t->win, t->melw,
                               t->meltask, t->nnz);
        });
    }
    CMOOP_HIP(hipGetLastError());
}

// Frames per workgroup of the stream kernels.  A workgroup's prologue (mel table into LDS, ~30 twiddle / window loads
// per lane) costs about as much as one frame of a wave, so a run should give every wave several frames; the grid should
// still hold at least two workgroups per compute unit so a 60 s recording (6 001 frames at hop 160) covers the chip.
// run = ceil(T / (2 CUs)) rounded up to the four waves, kept inside [8, 64].
int frontend_stream_run(int T, int compute_units) {
    const int64_t want = cdiv64((int64_t)T, 2 * (int64_t)std::max(1, compute_units));
    return (int)std::min<int64_t>(64, std::max<int64_t>(8, (want + 3) & ~(int64_t)3));
}

void launch_logmel_stream(const float* wav, int64_t n_samples, float* out, const FrontendTables* t, int compute_units, hipStream_t s) {
    const FrontendCfg& c = t->cfg;
    // frame * hop + n_fft stays inside int32 in the kernels' sample index
    CMOOP_REQUIRE(n_samples >= 1 && n_samples <= 0x7fffffffll - 2 * c.n_fft, "stream front end: 1 <= n_samples < 2^31 - 2 n_fft");
    const int T = frontend_frames(c, (int)n_samples);
    CMOOP_REQUIRE((int64_t)T * c.n_mels <= 0x7fffffff && T <= 0x7fffffff - 64, "stream front end: T * n_mels must stay below 2^31");
    CMOOP_REQUIRE(wav && out, "stream front end: NULL buffer");
    const int run = frontend_stream_run(T, compute_units);
    if (!t->general) {
        hipLaunchKernelGGL(logmel_stream_kernel, dim3((unsigned)cdiv(T, run)), dim3(256), 0, s, wav, (int)n_samples, out, T, run, c.hop,
                           c.n_mels, c.log_eps, t->tw, t->win, t->melw, t->meltask, t->nnz);
    } else {
        with_fft_points(c.n_fft, [&](auto nc) {
            hipLaunchKernelGGL(logmel_ex_stream_kernel<decltype(nc)::value>, dim3((unsigned)cdiv(T, run)), dim3(256), 0, s, wav,
                               (int)n_samples, out, T, run, c.hop, c.n_mels, c.scale, c.log_eps, c.db_amin, t->tw, t->win, t->melw,
                               t->meltask, t->nnz);
        });
    }
    CMOOP_HIP(hipGetLastError());
}

// ---- PCEN: per-channel energy normalisation of mel power (Wang et al. 2017; no reference counterpart) ---------------
// Per band, E[t] = input_scale P[t]:  M[t] = M[t-1] + s (E[t] - M[t-1]), M[-1] = E[0];
//                                     out[t] = (E[t] / (eps + M[t])^alpha + delta)^r - delta^r.
// The recurrence is serial in t and independent over bands, so every kernel gives a band (of a clip or of a chunk) to one
// thread with lanes on consecutive bands: a frame row is one coalesced access.
//   pcen_apply_kernel     clip form on a power tensor [n][T][F], one thread per (clip, band)
//   logmel_pcen_kernel    one launch from audio: the clip's workgroup stores power (logmel_ex_frames), barriers, then its
//                         first n_mels threads walk their own rows -- where the dB tail sits in logmel_ex_kernel
//   stream form, ONE recording [T][F] cut into chunks of `chunk` frames (pcen_stream_plan), three launches on one stream:
//     pcen_local_kernel   per (chunk, band): the smoother's state at the chunk's end from a zero start
//     pcen_carry_kernel   one workgroup, a thread per band, serial over chunks: carry[0] = E[0],
//                         carry[c+1] = a^chunk carry[c] + local[c]   (the update is linear in M: exact in real arithmetic)
//     pcen_apply_stream_kernel  per (chunk, band): the recurrence from carry[c], in place
//   The launches order themselves on the stream: no flags, no spinning, no atomics between workgroups.
// pcen_scale / pcen_step are the only arithmetic; contraction is off inside them so every kernel rounds alike.
__device__ __forceinline__ float pcen_scale(const PcenParams& p, const float P) {
#pragma clang fp contract(off)
    return p.input_scale * P;
}
// one frame: advances M and returns the output; dr = pcen_floor(p)
__device__ __forceinline__ float pcen_step(const PcenParams& p, const float dr, const float P, float& M) {
#pragma clang fp contract(off)
    const float E = pcen_scale(p, P);
    M = fmaf(p.s, E - M, M);
    return powf(E / powf(p.eps + M, p.alpha) + p.delta, p.r) - dr;
}
// delta^r by the call that raises the first term: E = 0 gives powf(0 + delta, r) - powf(delta, r) = 0.0f exactly
__device__ __forceinline__ float pcen_floor(const PcenParams& p) { return powf(p.delta, p.r); }

// `len` frames of one band column (rows [.][F]) from the state M, in place when WRITE (else only M advances: the output,
// and with it both powf, is dead code).  The chain is serial but its loads are not: eight frames are read ahead of it,
// which the compiler cannot do by itself past the stores.  The order of the arithmetic is the plain loop's.
constexpr int PCEN_AHEAD = 8;
template <bool WRITE, class Ptr>
__device__ __forceinline__ void pcen_run(const PcenParams& p, const float dr, Ptr col, const int len, const int F, float& M) {
    int t = 0;
    for (; t + PCEN_AHEAD <= len; t += PCEN_AHEAD) {
        float v[PCEN_AHEAD];
#pragma unroll
        for (int u = 0; u < PCEN_AHEAD; ++u) v[u] = col[(size_t)(t + u) * F];
#pragma unroll
        for (int u = 0; u < PCEN_AHEAD; ++u) {
            const float o = pcen_step(p, dr, v[u], M);
            if constexpr (WRITE) col[(size_t)(t + u) * F] = o;
        }
    }
    for (; t < len; ++t) {
        const float o = pcen_step(p, dr, col[(size_t)t * F], M);
        if constexpr (WRITE) col[(size_t)t * F] = o;
    }
}

// rows [.][F] of one band column: frames [0, T) from the state M[-1] = E[0]
__device__ __forceinline__ void pcen_walk(const PcenParams& p, float* col, int T, int F) {
    float M = pcen_scale(p, col[0]);
    pcen_run<true>(p, pcen_floor(p), col, T, F, M);
}

__global__ __launch_bounds__(256) void pcen_apply_kernel(PcenParams p, float* __restrict__ e, int cols, int T, int F) {
    const int g = blockIdx.x * 256 + threadIdx.x;                // (clip, band) = (g / F, g % F); cols = n F
    if (g >= cols) return;
    const int clip = g / F, band = g - clip * F;
    pcen_walk(p, e + (size_t)clip * T * F + band, T, F);
}

template <int NC>
__global__ __launch_bounds__(256) void logmel_pcen_kernel(const float* __restrict__ wav, int n_samples, float* __restrict__ out,
                                                          int T, int hop, int n_mels, PcenParams p,
                                                          const float* __restrict__ g_tw, const float* __restrict__ g_win,
                                                          const float* __restrict__ g_melw, const int* __restrict__ g_band,
                                                          int nnz) {
    float* rows = out + (size_t)blockIdx.x * T * n_mels;
    logmel_ex_frames<NC>(wav + (size_t)blockIdx.x * n_samples, n_samples, rows, 0, T, hop, n_mels, 2, 0.f, 0.f, g_tw, g_win, g_melw,
                         g_band, nnz);
    __syncthreads();                                             // orders the waves' stores of the power rows before the reads below
    if ((int)threadIdx.x < n_mels) pcen_walk(p, rows + threadIdx.x, T, n_mels);
}

__global__ __launch_bounds__(256) void pcen_local_kernel(PcenParams p, const float* __restrict__ e, float* __restrict__ local,
                                                         int T, int F, int chunk, int n_chunks) {
    const int g = blockIdx.x * 256 + threadIdx.x;                // (chunk, band) = (g / F, g % F)
    if (g >= (n_chunks - 1) * F) return;                         // the last chunk's end state is never read
    const int c = g / F, band = g - c * F;
    const float* col = e + (size_t)c * chunk * F + band;         // a full chunk: (c + 1) chunk < T
    float M = 0.f;
    pcen_run<false>(p, 0.f, col, chunk, F, M);
    local[g] = M;
}

__global__ __launch_bounds__(FRONTEND_MAX_MELS) void pcen_carry_kernel(PcenParams p, const float* __restrict__ e,
                                                                       const float* __restrict__ local, float* __restrict__ carry,
                                                                       int F, int n_chunks, float a_chunk) {
    const int band = threadIdx.x;
    if (band >= F) return;
    float M = pcen_scale(p, e[band]);
    carry[band] = M;
    int c = 0;
    constexpr int AHEAD = 32;                                    // the loads do not depend on the chain: 32 in flight at a time
    for (; c + AHEAD < n_chunks; c += AHEAD) {
        float l[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) l[u] = local[(size_t)(c + u) * F + band];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            M = fmaf(a_chunk, M, l[u]);
            carry[(size_t)(c + u + 1) * F + band] = M;
        }
    }
    for (; c + 1 < n_chunks; ++c) {
        M = fmaf(a_chunk, M, local[(size_t)c * F + band]);
        carry[(size_t)(c + 1) * F + band] = M;
    }
}

__global__ __launch_bounds__(256) void pcen_apply_stream_kernel(PcenParams p, float* __restrict__ e, const float* __restrict__ carry,
                                                                int T, int F, int chunk, int n_chunks) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_chunks * F) return;
    const int c = g / F, band = g - c * F;
    const int f0 = c * chunk, len = min(chunk, T - f0);
    float* col = e + (size_t)f0 * F + band;
    float M = carry[g];                                          // chunk 0: E[0], the clip form's start
    pcen_run<true>(p, pcen_floor(p), col, len, F, M);
}

void pcen_check(const PcenCfg& c) {
    auto fail = [](const char* field, const char* rule, double got) {
        throw std::runtime_error(std::string("pcen config: ") + field + " " + rule + " (got " + std::to_string(got) + ")");
    };
    if (!(c.s > 0.0 && c.s <= 1.0)) fail("s", "must satisfy 0 < s <= 1", c.s);
    if (!(c.alpha >= 0.0 && c.alpha <= 1.0)) fail("alpha", "must lie in [0, 1]", c.alpha);
    if (!(c.delta >= 0.0 && std::isfinite(c.delta))) fail("delta", "must be finite and not negative", c.delta);
    if (!(c.r > 0.0 && c.r <= 1.0)) fail("r", "must satisfy 0 < r <= 1", c.r);
    if (!(c.eps > 0.0 && std::isfinite(c.eps))) fail("eps", "must be finite and positive", c.eps);
    if (!(c.input_scale > 0.0 && std::isfinite(c.input_scale))) fail("input_scale", "must be finite and positive", c.input_scale);
    // the kernels compute in fp32: the rounded values must stay inside the domain too
    const PcenParams p = pcen_params(c);
    if (!(p.s > 0.f)) fail("s", "underflows fp32", c.s);
    if (!(p.r > 0.f)) fail("r", "underflows fp32", c.r);
    if (!(p.eps > 0.f)) fail("eps", "underflows fp32", c.eps);
    if (!(p.input_scale > 0.f && std::isfinite(p.input_scale))) fail("input_scale", "leaves the fp32 range", c.input_scale);
    if (!std::isfinite(p.delta)) fail("delta", "leaves the fp32 range", c.delta);
}

PcenParams pcen_params(const PcenCfg& c) {
    return PcenParams{(float)c.s, (float)c.alpha, (float)c.delta, (float)c.r, (float)c.eps, (float)c.input_scale};
}

double pcen_smoothing(double time_constant_s, int sr, int hop) {
    if (!(time_constant_s > 0.0 && std::isfinite(time_constant_s))) throw std::runtime_error("pcen smoothing: time_constant_s must be finite and positive");
    if (sr <= 0) throw std::runtime_error("pcen smoothing: sr must be positive");
    if (hop < 1) throw std::runtime_error("pcen smoothing: hop must be at least 1");
    const double tf = time_constant_s * (double)sr / (double)hop, tf2 = tf * tf;
    return (std::sqrt(1.0 + 4.0 * tf2) - 1.0) / (2.0 * tf2);
}

// chunk = ceil(sqrt(T)) / 4 rounded up to 64 frames, at least 64.  A frame of the apply pass is two powf (some hundreds
// of cycles), a chunk of the carry pass one dependent fma and a store (tens): the quarter keeps the two serial chains,
// `chunk` frames per thread and ceil(T / chunk) <= 4 sqrt(T) chunks in the carry pass's one workgroup, of comparable
// length, and short chunks put more threads on the chip (600 s at hop 160: 938 chunks of 64 frames; 64 up to 65 536 frames).
// A function of T alone: the chunking, and with it the bits, is the same on every device.
void pcen_stream_plan(int64_t n_frames, int* chunk, int* n_chunks) {
    CMOOP_REQUIRE(n_frames >= 1 && n_frames <= 0x7fffffff, "pcen stream plan: 1 <= n_frames < 2^31");
    int64_t root = (int64_t)std::sqrt((double)n_frames);
    while (root * root < n_frames) ++root;
    while (root > 1 && (root - 1) * (root - 1) >= n_frames) --root;
    const int64_t ch = std::max<int64_t>(PCEN_MIN_CHUNK, cdiv64(root, 4 * PCEN_MIN_CHUNK) * PCEN_MIN_CHUNK);
    if (chunk) *chunk = (int)ch;
    if (n_chunks) *n_chunks = (int)cdiv64(n_frames, ch);
}

static void pcen_shape_check(const char* who, int64_t n, int T, int F) {
    const std::string w(who);
    CMOOP_REQUIRE(F >= 1 && F <= FRONTEND_MAX_MELS, w + ": F must lie in 1..128 (got " + std::to_string(F) + ")");
    CMOOP_REQUIRE(T >= 1, w + ": T must be at least 1 (got " + std::to_string(T) + ")");
    CMOOP_REQUIRE(n >= 0 && n * (int64_t)T * F <= 0x7fffffffll - 256, w + ": n * T * F must stay below 2^31");
}

void launch_pcen_apply(const PcenParams& p, float* e, int64_t n, int T, int F, hipStream_t s) {
    pcen_shape_check("pcen_apply", n, T, F);
    if (n == 0) return;
    CMOOP_REQUIRE(e != nullptr, "pcen_apply: NULL buffer");
    const int cols = (int)(n * F);
    hipLaunchKernelGGL(pcen_apply_kernel, dim3((unsigned)cdiv(cols, 256)), dim3(256), 0, s, p, e, cols, T, F);
    CMOOP_HIP(hipGetLastError());
}

void launch_logmel_pcen(const float* wav, int64_t n_clips, int n_samples, float* out, const FrontendTables* t, const PcenParams& p,
                        hipStream_t s) {
    const FrontendCfg& c = t->cfg;
    CMOOP_REQUIRE(c.scale == 2 && t->general, "logmel_pcen: the front end config must have scale 2 (power)");
    const int T = frontend_frames(c, n_samples);
    CMOOP_REQUIRE(n_clips >= 0 && n_clips <= 0x7fffffff && (int64_t)T * c.n_mels <= 0x7fffffff, "front end: clip count / clip length out of range");
    if (n_clips == 0) return;
    CMOOP_REQUIRE(wav && out, "front end: NULL buffer");
    with_fft_points(c.n_fft, [&](auto nc) {
        hipLaunchKernelGGL(logmel_pcen_kernel<decltype(nc)::value>, dim3((unsigned)n_clips), dim3(256), 0, s, wav, n_samples, out, T,
                           c.hop, c.n_mels, p, t->tw, t->win, t->melw, t->meltask, t->nnz);
    });
    CMOOP_HIP(hipGetLastError());
}

size_t pcen_stream_workspace_floats(int T, int F) {
    int chunk = 0, n_chunks = 0;
    pcen_stream_plan(T, &chunk, &n_chunks);
    return (size_t)2 * n_chunks * F;                             // local | carry, each [n_chunks][F]
}

void launch_pcen_stream(const PcenParams& p, float* e, int T, int F, float* ws, hipStream_t s) {
    pcen_shape_check("pcen_stream", 1, T, F);
    CMOOP_REQUIRE(e && ws, "pcen_stream: NULL buffer");
    int chunk = 0, n_chunks = 0;
    pcen_stream_plan(T, &chunk, &n_chunks);
    float* local = ws;
    float* carry = ws + (size_t)n_chunks * F;
    const float a_chunk = (float)std::pow(1.0 - (double)p.s, (double)chunk);
    if (n_chunks > 1)
        hipLaunchKernelGGL(pcen_local_kernel, dim3((unsigned)cdiv((n_chunks - 1) * F, 256)), dim3(256), 0, s, p, e, local, T, F, chunk,
                           n_chunks);
    hipLaunchKernelGGL(pcen_carry_kernel, dim3(1), dim3(FRONTEND_MAX_MELS), 0, s, p, e, local, carry, F, n_chunks, a_chunk);
    hipLaunchKernelGGL(pcen_apply_stream_kernel, dim3((unsigned)cdiv(n_chunks * F, 256)), dim3(256), 0, s, p, e, carry, T, F, chunk,
                       n_chunks);
    CMOOP_HIP(hipGetLastError());
}

// MFCC option ("optional DCT-II ortho -> 40 MFCC"; the reference's own comment calls its features MFCCs,
// sa_nsga_init.py:68): out[row][k] = s_k * sum_f x[row][f] * cos(pi (f + 1/2) k / n), s_0 = sqrt(1/n), s_k = sqrt(2/n)
// -- scipy.fft.dct(type=2, norm="ortho") along the mel axis, first n_out coefficients.  HBM-bound (rows = clips x frames):
// a workgroup stages 32 rows and the n x n basis (built in double, once per workgroup) in LDS, 8 threads per row.
constexpr int MFCC_MAX = 64, MFCC_ROWS = 32;
__global__ __launch_bounds__(256) void mfcc_kernel(const float* __restrict__ X, float* __restrict__ Y, int64_t rows, int n,
                                                   int n_out) {
    __shared__ float basis[MFCC_MAX * (MFCC_MAX + 1)];
    __shared__ float xs[MFCC_ROWS * (MFCC_MAX + 1)];
    const int t = threadIdx.x;
    for (int i = t; i < n_out * n; i += 256) {
        const int k = i / n, f = i - k * n;
        const double sk = k == 0 ? sqrt(1.0 / n) : sqrt(2.0 / n);
        basis[k * (MFCC_MAX + 1) + f] = (float)(sk * cos(M_PI * (f + 0.5) * k / n));
    }
    const int64_t row0 = (int64_t)blockIdx.x * MFCC_ROWS;
    for (int i = t; i < MFCC_ROWS * n; i += 256) {
        const int r = i / n, f = i - r * n;
        xs[r * (MFCC_MAX + 1) + f] = row0 + r < rows ? X[(row0 + r) * n + f] : 0.f;
    }
    __syncthreads();
    const int r = t >> 3;
    if (row0 + r >= rows) return;
    for (int k = t & 7; k < n_out; k += 8) {
        float acc = 0.f;
        for (int f = 0; f < n; ++f) acc = fmaf(xs[r * (MFCC_MAX + 1) + f], basis[k * (MFCC_MAX + 1) + f], acc);
        Y[(row0 + r) * n_out + k] = acc;
    }
}

void launch_mfcc(const float* X, float* Y, int64_t rows, int n_mels, int n_mfcc, hipStream_t s) {
    CMOOP_REQUIRE(n_mels >= 1 && n_mels <= MFCC_MAX && n_mfcc >= 1 && n_mfcc <= n_mels, "mfcc: 1 <= n_mfcc <= n_mels <= 64");
    if (rows == 0) return;
    hipLaunchKernelGGL(mfcc_kernel, dim3((unsigned)cdiv64(rows, MFCC_ROWS)), dim3(256), 0, s, X, Y, rows, n_mels, n_mfcc);
    CMOOP_HIP(hipGetLastError());
}

// StandardScaler (nsga_penalty.py:103-141): mean / sqrt(biased var) per mel bin over N*T rows
__global__ void colstats_f64_kernel(const float* __restrict__ P, int blocks, int64_t M, int C, double* __restrict__ mean,
                                    double* __restrict__ scale) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < blocks; ++b) {
        s1 += (double)P[(size_t)b * 2 * C + c];
        s2 += (double)P[(size_t)b * 2 * C + C + c];
    }
    const double mu = s1 / (double)M;
    double var = s2 / (double)M - mu * mu;
    if (var < 0.0) var = 0.0;
    double sc = sqrt(var);
    if (sc == 0.0) sc = 1.0;
    mean[c] = mu;
    scale[c] = sc;
}

void colstats_finalize_f64(const float* P, int blocks, int64_t M, int C, double* mean, double* scale, hipStream_t s) {
    hipLaunchKernelGGL(colstats_f64_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, P, blocks, M, C, mean, scale);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void standardize_kernel(float* __restrict__ X, const double* __restrict__ mean,
                                                          const double* __restrict__ scale, int64_t n, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        X[i] = (float)(((double)X[i] - mean[c]) / scale[c]);
    }
}

void launch_standardize(float* X, const double* mean, const double* scale, int64_t rows, int C, hipStream_t s) {
    const int64_t n = rows * C;
    if (n == 0) return;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n, 256), 16384));
    hipLaunchKernelGGL(standardize_kernel, dim3(grid), dim3(256), 0, s, X, mean, scale, n, C);
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
