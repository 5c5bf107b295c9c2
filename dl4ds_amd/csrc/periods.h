// What the time-axis walks share (indices.hip, temporal.hip, extremes.hip's pot_peaks): the periods of the time axis, given by the
// host array period_starts with P + 1 entries (int64, strictly increasing, first 0, last N) and read by the kernels from the front
// of the workspace; the fp32 validity test; the comparison op of the thresholds.
#pragma once
#include "common.h"

// a valid sample, a usable threshold: false for NaN and +-inf
__device__ __forceinline__ bool finite_f32(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// op 0 >=, 1 >, 2 <, 3 <=: x < t is -x > -t and x <= t is -x >= -t (exact), so the kernels negate both sides and compare upwards
struct CmpOp {
    bool neg, strict;
};
__device__ __forceinline__ CmpOp decode_op(int op) { return {op >= 2, op == 1 || op == 2}; }

// refuses period starts that are not P + 1 strictly increasing entries from 0 to N (P >= 1); `entry` names the caller in the message
inline void check_period_starts(const char* entry, const long long* period_starts, int P, size_t N) {
    const std::string who(entry);
    DL4DS_REQUIRE(period_starts, who + ": null period starts");
    DL4DS_REQUIRE((size_t)P <= N && period_starts[0] == 0 && period_starts[P] == (long long)N,
                  who + ": period starts must be strictly increasing from 0 to N");
    for (int p = 0; p < P; ++p)
        DL4DS_REQUIRE(period_starts[p + 1] > period_starts[p], who + ": period starts must be strictly increasing from 0 to N");
}

inline size_t period_starts_bytes(int P) { return ((size_t)P + 1) * sizeof(long long); }

// the starts at the front of the workspace, for the kernels; waits for the copy (and for whatever else the stream holds): the
// caller's array may go away after the call
inline const long long* upload_period_starts(hipStream_t s, const long long* period_starts, int P, void* workspace) {
    HIP_CHECK(hipMemcpyAsync(workspace, period_starts, period_starts_bytes(P), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return static_cast<const long long*>(workspace);
}
