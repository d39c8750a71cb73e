// What the five chip-cutting files (chips.hip, s2_chips.hip, raster_chips.hip, s2_raster_chips.hip, s1_chips.hip) share beside the
// column kernels' last phase (chip_epilogue.h) and the segment access (pixel_seg.h): the "any" collapse of the date masks of the two
// segment kernels, the 2^40 limit, and the argument checks common to the entry points.  The other repeated device
// text stays in the kernels: shared helpers changed their registers or scratch (profiles/chip_layer_refactor.txt).
#pragma once
#include "chip_epilogue.h"
#include "common.h"
#include "pixel_seg.h"

namespace {

constexpr int CHIP_MAX_T = 32;         // dates: one bit each in the per-pixel date mask
constexpr long CHIP_LIM40 = 1L << 40;  // elements of one output

// strategy "any": a pixel masked on one date is masked on all
template <int N>
__device__ __forceinline__ void any_date(unsigned (&dm)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) dm[j] = dm[j] ? 0xffffffffu : 0u;
}

// ---- the entry points' common argument checks: `fn` is the entry point's name; a failed check sets the error and yields IG_ERR_ARG ----
#define CHIP_CHECK(call) do { const int rc_ = (call); if (rc_ != IG_OK) return rc_; } while (0)

inline int chip_check_stack(const char* fn, int n, int T, int C) {
    IG_REQUIRE(n >= 0, "%s: need n >= 0 (got %d)", fn, n);
    IG_REQUIRE(T >= 1 && T <= CHIP_MAX_T, "%s: 1 <= T <= %d dates (got %d)", fn, CHIP_MAX_T, T);
    IG_REQUIRE(C >= 1, "%s: need C >= 1 bands per date (got %d)", fn, C);
    return IG_OK;
}

inline int chip_check_side(const char* fn, int S) {  // the column kernels'
    IG_REQUIRE(S >= 1 && S <= (1 << 15), "%s: need a chip side 1 <= S <= 2^15 (got %d)", fn, S);
    return IG_OK;
}

inline int chip_check_strategy(const char* fn, int strategy) {
    IG_REQUIRE(strategy == 0 || strategy == 1, "%s: strategy must be 0 each or 1 any (got %d)", fn, strategy);
    return IG_OK;
}

inline int chip_check_hls_rule(const char* fn, int mask_bits, int strategy, int no_data, int clip, int clip_lo, int clip_hi) {
    IG_REQUIRE(mask_bits >= 0 && mask_bits <= 255, "%s: mask_bits must be a byte (got %d)", fn, mask_bits);
    CHIP_CHECK(chip_check_strategy(fn, strategy));
    IG_REQUIRE(no_data >= -32768 && no_data <= 32767, "%s: no_data must fit int16 (got %d)", fn, no_data);
    IG_REQUIRE(clip == 0 || clip == 1, "%s: clip must be 0 or 1 (got %d)", fn, clip);
    IG_REQUIRE(!clip || (clip_lo >= -32768 && clip_hi <= 32767 && clip_lo <= clip_hi),
               "%s: the clip range must fit int16 with clip_lo <= clip_hi (got %d, %d)", fn, clip_lo, clip_hi);
    return IG_OK;
}

inline int chip_check_s2_rule(const char* fn, int strategy, int no_data, int boa_offset, int range, int range_lo, int range_hi) {
    CHIP_CHECK(chip_check_strategy(fn, strategy));
    IG_REQUIRE(no_data >= 0 && no_data <= 65535, "%s: no_data must fit uint16 (got %d)", fn, no_data);
    IG_REQUIRE(boa_offset >= 0 && boa_offset <= 65535, "%s: boa_offset must lie in [0, 65535] (got %d)", fn, boa_offset);
    IG_REQUIRE(range == 0 || range == 1, "%s: range must be 0 or 1 (got %d)", fn, range);
    IG_REQUIRE(!range || (range_lo >= 0 && range_hi <= 65535 && range_lo <= range_hi),
               "%s: the valid range must fit uint16 with range_lo <= range_hi (got %d, %d)", fn, range_lo, range_hi);
    return IG_OK;
}

inline int chip_check_labels(const char* fn, int elem_size, int valid_bit, int K) {
    IG_REQUIRE(elem_size == 1 || elem_size == 4, "%s: elem_size must be 1 (int8) or 4 (float32) (got %d)", fn, elem_size);
    IG_REQUIRE(valid_bit >= 0 && valid_bit <= 2, "%s: valid_bit must be 0 none, 1 any or 2 each (got %d)", fn, valid_bit);
    IG_REQUIRE(K >= 0 && K <= EPI_MAX_K, "%s: need 0 <= K <= %d histogram cells (got %d)", fn, EPI_MAX_K, K);
    IG_REQUIRE(K == 0 || elem_size == 1, "%s: a class histogram (K = %d) needs int8 labels", fn, K);
    return IG_OK;
}

// the values of one chip (TC = T * C planes), before the entry point returns for n == 0
inline int chip_check_values(const char* fn, long TC, int S) {
    IG_REQUIRE(TC * S * S <= 0x7fffffffL, "%s: T * C * S * S = %ld values per chip exceeds 2^31 - 1 (valid_values is int32)", fn, TC * S * S);
    return IG_OK;
}

// the values and the workgroups (per: of one chip) of n >= 1 chips
inline int chip_check_launch(const char* fn, int n, long TC, int S, long per) {
    IG_REQUIRE(TC * S * S < CHIP_LIM40 / n, "%s: n * T * C * S * S exceeds 2^40 values (n %d, S %d)", fn, n, S);
    IG_REQUIRE(per * n <= 0x7fffffffL, "%s: %ld workgroups exceed 2^31 - 1 (n %d, S %d)", fn, per * n, n, S);
    return IG_OK;
}

}  // namespace
