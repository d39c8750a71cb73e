// Post-hoc calibration of the segmentation logits for gfx950: the cross-entropy at a whole grid of temperatures in one
// pass over the logits, and reliability histograms of the top-class confidence at one temperature.  Not in the reference.
//   calib_nll_kernel    nll[k] += sum over valid pixels of logsumexp_c(beta_k z_c) - beta_k z_y,  k < K <= 32
//   calib_fold_kernel   the ordered fold of the per-workgroup partials into nll
//   reliability_kernel  hist[pred][{n, hits, conf sum in 2^-24 units}][bin] of conf = max softmax(beta z)
// logits (B, ncls, HW) f32 planar, 2 <= ncls <= 127: a thread owns pixels (consecutive lanes read consecutive addresses of one class
// plane); the classes are walked twice with a run-time trip count and NO per-thread class array -- pass A finds the maximum, the first
// argmax and the label's logit, pass B re-reads each z_c (an L1 / L2 hit) and adds exp2(beta_k log2e (z_c - m)) to K accumulators in
// registers (compile-time unrolled; the beta_k arrive by value in the kernel argument, i.e. in SGPRs).
// Valid pixel: valid_label (pixel_logits.h), the rule of ig_ce_loss.
//
// Determinism.  calib_nll_kernel: a thread adds its pixels' terms in double in pixel order, the wave and the workgroup are reduced in a
// fixed pattern, workgroup b stores its K partials (and its sum of max - z_y, the part of the loss that is linear in beta) to
// scratch[b][.]; calib_fold_kernel (one workgroup) adds them in workgroup order (8 strided subsets per column, folded in subset
// order) and does nll[k] += total_k + beta_k * total_dy.  The grid depends on the shape only: the bits repeat from
// run to run.  The count and the histograms are integers (LDS adds, then one global add per non-empty cell and workgroup).
#include "common.h"
#include "pixel_logits.h"

namespace {

constexpr int TPB = PX_TPB, NWAVE = PX_NWAVE;
constexpr int MAX_K = 32, NCOL = MAX_K + 1, MAX_WG = PX_MAX_WG, FOLD_SUB = 8;  // a partial row: K sums + the sum of (max - z_y)
constexpr int MAX_NCLS = 127, MAX_BINS = 64, MAX_CELLS = 4096;
constexpr double LOG2E = 1.44269504088896340736;

struct Betas {
    float l2[MAX_K];  // beta_k * log2(e), rounded once from double; entries K.. repeat entry 0 (computed, never stored)
};
struct BetasD {
    double b[MAX_K];
};

// class 0's logit of pixel m; class c is c * HW floats further on
__device__ __forceinline__ const float* pixel_base(const float* logits, long m, long HW, int ncls) {
    long b, pix;
    split_pixel(m, HW, b, pix);
    return logits + b * ncls * HW + pix;
}

template <typename LABEL, int KT>
__global__ __launch_bounds__(TPB) void calib_nll_kernel(const float* __restrict__ logits, const LABEL* __restrict__ labels, long ignore_index,
                                                        Betas beta, double* __restrict__ part, unsigned long long* __restrict__ count, long M,
                                                        long HW, int ncls) {
    __shared__ unsigned cnt[NWAVE];
    double acc[KT + 1];  // [k < KT] sum of log(sum_c exp(beta_k (z_c - m))); [KT] sum of (m - z_y), which beta_k multiplies in the fold
#pragma unroll
    for (int k = 0; k <= KT; ++k) acc[k] = 0.0;
    unsigned n = 0;
    for (long m = blockIdx.x * (long)TPB + threadIdx.x; m < M; m += (long)gridDim.x * TPB) {
        int y;
        if (!valid_label(labels, m, ignore_index, ncls, y)) continue;
        const float* z = pixel_base(logits, m, HW, ncls);
        float mx = -INFINITY, zy = 0.f;
        int am = 0;
        for (int c = 0; c < ncls; ++c) {  // pass A
            const float v = z[(long)c * HW];
            if (v > mx) mx = v, am = c;
            if (c == y) zy = v;
        }
        // the first maximum contributes exp2(0) = 1 exactly: it is left out of the sum and comes back through log1p, which keeps the
        // small loss of a confident pixel (sum = 1 + 1e-9) instead of rounding it away
        float s[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) s[k] = 0.f;
        for (int c = 0; c < ncls; ++c) {  // pass B
            const float d = z[(long)c * HW] - mx;
            if (c == am) continue;
#pragma unroll
            for (int k = 0; k < KT; ++k) s[k] += __builtin_amdgcn_exp2f(beta.l2[k] * d);
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] += (double)log1pf(s[k]);
        acc[KT] += (double)(mx - zy);  // >= 0
        ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n;
    const double t = block_totals<KT + 1>(acc);  // its barrier also publishes cnt
    if (threadIdx.x <= KT) part[(size_t)blockIdx.x * NCOL + (threadIdx.x < KT ? threadIdx.x : MAX_K)] = t;
    if (threadIdx.x == 0) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) c += cnt[w];
        if (c) atomicAdd(count, c);
    }
}

// one workgroup of FOLD_SUB * 64 threads: thread (g, k) adds column k of the partials of workgroups g, g + FOLD_SUB, ... in that order;
// nll[k] += (column k) + beta_k * (column MAX_K)
__global__ __launch_bounds__(FOLD_SUB * 64) void calib_fold_kernel(const double* __restrict__ part, double* __restrict__ nll, BetasD beta, int nblk,
                                                                   int K) {
    __shared__ double sub[FOLD_SUB][NCOL];
    const int k = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (k < NCOL) {
        double a = 0.0;
        if (k < K || k == MAX_K)
            for (int b = g; b < nblk; b += FOLD_SUB) a += part[(size_t)b * NCOL + k];
        sub[g][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = 0.0, d = 0.0;
#pragma unroll
        for (int q = 0; q < FOLD_SUB; ++q) t += sub[q][threadIdx.x], d += sub[q][MAX_K];
        nll[threadIdx.x] += t + beta.b[threadIdx.x] * d;
    }
}

// LDS: cells = ncls * nbins; u32 n[cells], u32 hit[cells], then u64 conf[cells] (8-byte aligned: 8 * cells bytes in front of it).
// A workgroup sees at most 2^40 / MAX_WG = 2^30 pixels (checked by the entry point): the u32 cells cannot wrap.
template <typename LABEL>
__global__ __launch_bounds__(TPB) void reliability_kernel(const float* __restrict__ logits, const LABEL* __restrict__ labels, long ignore_index,
                                                          float beta_l2, unsigned long long* __restrict__ hist, long M, long HW, int ncls,
                                                          int nbins) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int cells = ncls * nbins;
    unsigned* s_n = reinterpret_cast<unsigned*>(smem);
    unsigned* s_hit = s_n + cells;
    unsigned long long* s_conf = reinterpret_cast<unsigned long long*>(s_hit + cells);
    for (int i = threadIdx.x; i < cells; i += TPB) s_n[i] = 0u, s_hit[i] = 0u, s_conf[i] = 0ull;
    __syncthreads();
    const float fb = (float)nbins;
    for (long m = blockIdx.x * (long)TPB + threadIdx.x; m < M; m += (long)gridDim.x * TPB) {
        int y;
        if (!valid_label(labels, m, ignore_index, ncls, y)) continue;
        const float* z = pixel_base(logits, m, HW, ncls);
        float mx = -INFINITY;
        int am = 0;
        for (int c = 0; c < ncls; ++c) {
            const float v = z[(long)c * HW];
            if (v > mx) mx = v, am = c;  // the first maximum: ig_argmax_i8's rule
        }
        float s = 0.f;
        for (int c = 0; c < ncls; ++c) {
            const float d = z[(long)c * HW] - mx;
            if (c != am) s += __builtin_amdgcn_exp2f(beta_l2 * d);
        }
        const float conf = 1.f / (1.f + s);  // p[pred] = exp(0) / sum; in [1 / ncls, 1]
        int bin = (int)(conf * fb);
        bin = bin < 0 ? 0 : bin > nbins - 1 ? nbins - 1 : bin;  // conf = 1 belongs to the top bin; a NaN (non-finite logits) lands in bin 0
        const int cell = am * nbins + bin;                      // am < ncls and bin < nbins: inside the LDS table
        const double q = (double)conf * 16777216.0 + 0.5;       // exact in double: floor(conf * 2^24 + 0.5)
        atomicAdd(s_n + cell, 1u);
        if (am == y) atomicAdd(s_hit + cell, 1u);
        atomicAdd(s_conf + cell, q >= 0.5 ? (unsigned long long)q : 0ull);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += TPB) {
        const unsigned cn = s_n[i];
        if (!cn) continue;
        unsigned long long* h = hist + ((size_t)(i / nbins) * 3) * nbins + i % nbins;  // [pred][3][nbins]
        atomicAdd(h, (unsigned long long)cn);
        if (s_hit[i]) atomicAdd(h + nbins, (unsigned long long)s_hit[i]);
        if (s_conf[i]) atomicAdd(h + 2 * nbins, s_conf[i]);
    }
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define IG_REQUIRE_PIXELS(name)                                                                                                   \
    IG_REQUIRE(ncls >= 2 && ncls <= MAX_NCLS, name ": 2 <= ncls <= %d (got %d)", MAX_NCLS, ncls);                                 \
    IG_REQUIRE(B >= 0 && HW >= 0, name ": negative size (B %d, HW %ld)", B, HW);                                                  \
    IG_REQUIRE(label_dtype >= 0 && label_dtype <= 2, name ": label_dtype must be 0 (int64), 1 (int32) or 2 (float32) (got %d)", label_dtype)

extern "C" {

int ig_calib_nll_grid(const float* logits, const void* labels, int label_dtype, long ignore_index, const float* inv_temps, int K, double* nll,
                      unsigned long long* count, int B, long HW, int ncls, void* stream) {
    IG_REQUIRE(K >= 1 && K <= MAX_K, "ig_calib_nll_grid: 1 <= K <= %d (got %d)", MAX_K, K);
    IG_REQUIRE(inv_temps, "ig_calib_nll_grid: null pointer (inv_temps)");
    for (int k = 0; k < K; ++k)
        IG_REQUIRE(inv_temps[k] > 0.f && inv_temps[k] <= 3.0e38f, "ig_calib_nll_grid: inv_temps[%d] = %g is not a finite positive number", k,
                   (double)inv_temps[k]);
    IG_REQUIRE_PIXELS("ig_calib_nll_grid");
    const long M = (long)B * HW;
    if (M == 0) return IG_OK;
    IG_REQUIRE(logits && labels && nll && count, "ig_calib_nll_grid: null pointer");
    Betas beta;
    BetasD beta_d;
    for (int k = 0; k < MAX_K; ++k) {
        beta_d.b[k] = (double)inv_temps[k < K ? k : 0];
        beta.l2[k] = (float)(beta_d.b[k] * LOG2E);
    }
    const int nblk = pixel_grid(M);
    double* part = (double*)ig_scratch(IG_SLOT_CALIB_NLL, (size_t)MAX_WG * NCOL * sizeof(double), ST(stream));
    IG_REQUIRE(part, "ig_calib_nll_grid: scratch allocation failed");
    const int rc = ig_label_dispatch(label_dtype, [&](auto tag) {
        using LT = typename decltype(tag)::type;
        auto nll_k = [&](auto kt) {
            return ig_launch<calib_nll_kernel<LT, decltype(kt)::value>>("ig_calib_nll_grid", dim3((unsigned)nblk), dim3(TPB), 0, ST(stream), logits,
                                                                        (const LT*)labels, ignore_index, beta, part, count, M, HW, ncls);
        };
        if (K <= 4) return nll_k(IntTag<4>{});
        if (K <= 8) return nll_k(IntTag<8>{});
        if (K <= 16) return nll_k(IntTag<16>{});
        return nll_k(IntTag<32>{});
    });
    if (rc != IG_OK) return rc;
    return ig_launch<calib_fold_kernel>("ig_calib_nll_grid", dim3(1), dim3(FOLD_SUB * 64), 0, ST(stream), part, nll, beta_d, nblk, K);
}

int ig_reliability_update(const float* logits, const void* labels, int label_dtype, long ignore_index, float inv_temp, unsigned long long* hist,
                          int B, long HW, int ncls, int nbins, void* stream) {
    IG_REQUIRE(inv_temp > 0.f && inv_temp <= 3.0e38f, "ig_reliability_update: inv_temp = %g is not a finite positive number", (double)inv_temp);
    IG_REQUIRE(nbins >= 1 && nbins <= MAX_BINS, "ig_reliability_update: 1 <= nbins <= %d (got %d)", MAX_BINS, nbins);
    IG_REQUIRE_PIXELS("ig_reliability_update");
    IG_REQUIRE(ncls * nbins <= MAX_CELLS, "ig_reliability_update: ncls * nbins = %d x %d exceeds %d cells (the workgroup's LDS histogram)", ncls,
               nbins, MAX_CELLS);
    const long M = (long)B * HW;
    if (M == 0) return IG_OK;
    IG_REQUIRE(M <= (1L << 40), "ig_reliability_update: B * HW = %ld exceeds 2^40 pixels per call (32-bit LDS counts)", M);
    IG_REQUIRE(logits && labels && hist, "ig_reliability_update: null pointer");
    const int nblk = pixel_grid(M), smem = ncls * nbins * 16;
    const float bl2 = (float)((double)inv_temp * LOG2E);
    return ig_label_dispatch(label_dtype, [&](auto tag) {
        using LT = typename decltype(tag)::type;
        return ig_launch<reliability_kernel<LT>>("ig_reliability_update", dim3((unsigned)nblk), dim3(TPB), smem, ST(stream), logits, (const LT*)labels,
                                                 ignore_index, bl2, hist, M, HW, ncls, nbins);
    });
}

}  // extern "C"
