// Host-side planner of the I/O adaptor (sva_io_*): the polyphase tables of audio_io.resample (torchaudio 2.4 sinc_interp_hann, width 6,
// rolloff 0.99), the per-sample readiness rule, and the counters of a stream that is fed blocks of any length at io_rate while the engine
// consumes whole chunks at 44.1 kHz.  Pure arithmetic on host integers -- no HIP, no sva_batch: the engine executes exactly what IoPlan::push
// returns, and tests/test_io_plan.py pins it without a GPU through sva_test_io_plan.
//
//   one direction (orig : new, reduced):   y[i * new + p] = sum_t K[p][t] * x[i * orig - width + t],   t = 0 .. 2 * width + orig - 1
//   Taps whose clipped argument sits at +-6 carry the window's cos^2(pi / 2) ~ 4e-33: they are left out, phase p keeps taps lo[p] .. hi[p],
//   and need(j) = i * orig - width + hi[p] is the last input index output j reads.  Output j exists as soon as need(j) has been received.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sva {

constexpr int kIoModelRate = 44100;
constexpr int kIoMaxRatioTerm = 640;       // the reduced orig and new of an accepted rate are both <= this
constexpr int kIoMinRate = 8000, kIoMaxRate = 96000;
constexpr int kIoLowpassWidth = 6;
constexpr double kIoRolloff = 0.99;

inline long long io_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// one direction of the resampler
struct ResampleTable {
    int orig = 1, new_ = 1, width = 0, taps = 1;
    int support = 1;                       // max over phases of hi - lo + 1
    bool identity = true;                  // orig == new: samples are copied, no filter runs
    std::vector<int> lo, hi;               // [new]
    std::vector<float> k;                  // [support][new]: k[s * new + p] = K[p][lo[p] + s] rounded once to fp32 (0 past hi[p]); adjacent lanes
                                           // of the kernels hold adjacent phases, so a row of this layout is one coalesced read

    void build(int from_rate, int to_rate) {
        const int g = (int)io_gcd(from_rate, to_rate);
        orig = from_rate / g; new_ = to_rate / g;
        identity = orig == new_;
        if (identity) { width = 0; taps = 1; support = 1; lo.assign(1, 0); hi.assign(1, 0); k.assign(1, 1.f); return; }
        // the operations of _sinc_resample_kernel in its order, so the clip decides the same taps here and there
        const double base_freq = std::min(orig, new_) * kIoRolloff;
        width = (int)ceil(kIoLowpassWidth * (double)orig / base_freq);
        taps = 2 * width + orig;
        lo.assign(new_, taps); hi.assign(new_, -1);
        std::vector<double> k64((size_t)new_ * taps, 0.0);      // [new][taps], every tap: what _sinc_resample_kernel returns
        const double scale = base_freq / orig;
        for (int p = 0; p < new_; ++p)
            for (int t = 0; t < taps; ++t) {
                double a = ((double)(-p) / new_ + (double)(t - width) / orig) * base_freq;
                a = std::min(std::max(a, (double)-kIoLowpassWidth), (double)kIoLowpassWidth);
                const double c = cos(a * M_PI / kIoLowpassWidth / 2);
                const double w = c * c, x = a * M_PI;
                k64[(size_t)p * taps + t] = (x == 0 ? 1.0 : sin(x) / x) * w * scale;
                if (a > -kIoLowpassWidth && a < kIoLowpassWidth) { lo[p] = std::min(lo[p], t); hi[p] = std::max(hi[p], t); }
            }
        support = 0;
        for (int p = 0; p < new_; ++p) support = std::max(support, hi[p] - lo[p] + 1);
        k.assign((size_t)support * new_, 0.f);
        for (int p = 0; p < new_; ++p)
            for (int t = lo[p]; t <= hi[p]; ++t) k[(size_t)(t - lo[p]) * new_ + p] = (float)k64[(size_t)p * taps + t];
    }
    // last input index output j reads
    long long need(long long j) const { const int p = (int)(j % new_); return (j / new_) * orig - width + hi[p]; }
    // need() never decreases with j (the engine and the kernels rely on it: the ready outputs are a prefix)
    bool monotone() const {
        for (int p = 0; p + 1 < new_; ++p) if (hi[p + 1] < hi[p] || lo[p + 1] < lo[p]) return false;
        return hi[0] + orig >= hi[new_ - 1] && lo[0] + orig >= lo[new_ - 1];
    }
    // outputs ready once n inputs have been received: the count of j with need(j) < n
    long long ready(long long n) const {
        if (n <= 0) return 0;
        long long i = (n - 1 + width - hi[0]) / orig - 2;          // every phase of the blocks before this one is ready
        long long j = std::max(0LL, i) * new_;
        while (need(j) < n) ++j;
        return j;
    }
    // history the kernels keep: an output that is not ready at n starts above n - taps
    int history() const { return taps; }
};

inline bool io_rate_supported(int io_rate) {
    if (io_rate < kIoMinRate || io_rate > kIoMaxRate) return false;
    const int g = (int)io_gcd(io_rate, kIoModelRate);
    return io_rate / g <= kIoMaxRatioTerm && kIoModelRate / g <= kIoMaxRatioTerm;
}
constexpr const char* kIoRateRule =
    "io_rate must be an integer in 8000 .. 96000 whose ratio to 44100, reduced by their gcd, has both terms <= 640";

// what one call of n samples does
struct IoCall {
    long long m0 = 0, m1 = 0;              // model-rate samples [m0, m1) become ready
    int steps = 0;                         // engine steps to run
    long long r0 = 0, r1 = 0;              // io-rate samples [r0, r1) are produced by those steps
    int in_fill = 0;                       // model-rate samples staged and not yet consumed, after the call
    int out_fill = 0;                      // io-rate samples in the output FIFO after the call's n have been popped
};

struct IoPlan {
    int io_rate = kIoModelRate, chunk = 2048, max_block = 0;
    ResampleTable in, out;                 // io_rate -> 44100, 44100 -> io_rate
    int L = 0, L_filter = 0;               // latency in io-rate samples; the part of it that is filter delay
    int nbuf = 0;                          // chunk staging buffers
    int hist_in = 0, hist_out = 0;         // history samples kept per slot, at io_rate and at 44100
    int fifo_cap = 0;                      // output FIFO samples per slot
    int stage_cap = 0;                     // = nbuf * chunk
    long long period = 0;                  // every counter repeats its pattern with this many pushed samples
    // running totals
    long long N = 0, M = 0, S = 0, R = 0;  // pushed, model-rate ready, steps run, io-rate produced

    // With r(N) the io-rate samples that exist once N have been pushed (an engine that consumes `chunk_` samples per step): the smallest L with
    // r(N) + L >= N for every N, and the max over N of r(N) + L - N.  The counters repeat with `per` pushed samples once both
    // filters have left their start-up (the first step has run: a chunk at io_rate -- at most a period -- plus the look-ahead); one sweep over
    // that start-up and a whole period behind it sees every value.  Sample by sample on the host: 10-45 ms at chunk_frames 1-4, about 0.7 s
    // at 64 (48 kHz) -- paid once, at open
    void sweep(int chunk_, int* L_out, long long* surplus_out) const {
        const long long per = (long long)in.orig * (chunk_ / io_gcd(in.new_, chunk_));
        long long jm = 0, r = 0, Lmax = 0, smax = 0;
        const long long n_end = 3 * per + 2 * in.taps + ((long long)out.taps * in.orig) / in.new_ + 2;
        for (long long n = 0; n <= n_end; ++n) {
            while (in.need(jm) < n) ++jm;
            const long long y = (jm / chunk_) * chunk_;
            while (out.need(r) < y) ++r;
            Lmax = std::max(Lmax, n - r);
            smax = std::max(smax, r - n);
        }
        *L_out = (int)Lmax;
        if (surplus_out) *surplus_out = smax + Lmax;
    }
    // false: unsupported rate (kIoRateRule)
    bool open(int io_rate_, int chunk_frames, int max_block_) {
        if (!io_rate_supported(io_rate_) || chunk_frames < 1 || max_block_ < 1) return false;
        io_rate = io_rate_; chunk = 2048 * chunk_frames; max_block = max_block_;
        in.build(io_rate, kIoModelRate);
        out.build(kIoModelRate, io_rate);
        if (!in.monotone() || !out.monotone()) return false;
        period = (long long)in.orig * (chunk / io_gcd(in.new_, chunk));
        long long surplus = 0;
        sweep(chunk, &L, &surplus);
        sweep(1, &L_filter, nullptr);
        hist_in = in.history();
        hist_out = out.history();
        // one call makes at most this many model-rate samples ready; they land in the chunk being filled and the ones after it
        const long long m_call = ((long long)max_block * in.new_ + in.orig - 1) / in.orig + 1;
        nbuf = (int)(m_call / chunk) + 2;
        stage_cap = nbuf * chunk;
        // before the pop the FIFO holds at most what it held after the last pop plus what this call's steps produced
        fifo_cap = (int)surplus + max_block + 1;
        N = M = S = R = 0;
        return true;
    }
    IoCall push(int n) {
        IoCall c;
        c.m0 = M;
        N += n;
        M = in.ready(N);
        c.m1 = M;
        const long long s1 = M / chunk;
        c.steps = (int)(s1 - S);
        S = s1;
        c.r0 = R;
        R = out.ready(S * chunk);
        c.r1 = R;
        c.in_fill = (int)(M - S * chunk);
        c.out_fill = (int)(R + L - N);
        return c;
    }
};

}  // namespace sva
