// fic_ctx_options.h -- the option names the handles share (fic_ctx_set_option, fic_rgb_ctx_set_option, fic_qt_ctx_set_option of
// include/fic.h), each with its range and the words of its refusal, once.  Plain C++ without HIP: set_core_option
// (fic_ctx_core.cpp) applies a rule to a context's core, tests/cpp/ctx_options_test.cpp walks the table under the address and
// undefined-behaviour sanitizers.  What only one handle knows ("sweep", "q_shape", "q_noflag") stays in its own entry.
#pragma once
#include <limits.h>
#include <string.h>

enum OptHandle { kOptGrey = 1, kOptRgb = 2, kOptQt = 4 };   // which handle asks; a rule lists the ones that know its name
enum OptId { kOptSearch, kOptChunks, kOptQEshift, kOptLsqTauWiden, kOptLsqEngine, kOptLsqQEshift, kOptTimeSweep, kOptSweepStats };

struct OptionRule {
    const char* name;
    int handles;         // OptHandle bits
    OptId id;
    int lo, hi;          // accepted: lo..hi
    bool zero_too;       // and 0, outside lo..hi
    const char* must;    // the refusal reads "<name> <must>" behind the entry's prefix
};

constexpr OptionRule kOptionRules[] = {
    {"search", kOptGrey | kOptRgb | kOptQt, kOptSearch, 0, 1, false, "must be 0 (the reference's criterion) or 1 (least squares)"},
    {"chunks", kOptGrey | kOptRgb, kOptChunks, 0, INT_MAX, false, "must be >= 0"},
    // diagnostics: values above 0 give WRONG codebooks (the matrix-core sweep's E_r times 2^-value; the fast least-squares
    // sweep's tau times 1 + 2^-value; the matrix-core least-squares sweep's Er times 2^-value)
    {"q_eshift", kOptGrey | kOptRgb, kOptQEshift, -12, 4, false, "must be in -12..4"},
    {"lsq_tau_widen", kOptGrey | kOptRgb, kOptLsqTauWiden, 8, 24, true, "must be 0 (off) or in 8..24"},
    // which sweep a full least-squares search runs: the two handles name their own kernels
    {"lsq_engine", kOptGrey, kOptLsqEngine, 0, 1, false, "must be 0 (VALU, k_sweep_lsq_fast) or 1 (matrix cores, k_sweep_lsq_q)"},
    {"lsq_engine", kOptRgb, kOptLsqEngine, 0, 1, false, "must be 0 (VALU sweeps) or 1 (matrix cores, k_sweep_lsq_rgb_q)"},
    {"lsq_q_eshift", kOptGrey | kOptRgb, kOptLsqQEshift, -12, 4, false, "must be in -12..4"},
    // switches: any value, non-zero is on
    {"time_sweep", kOptGrey | kOptRgb, kOptTimeSweep, INT_MIN, INT_MAX, false, ""},
    {"sweep_stats", kOptGrey | kOptRgb, kOptSweepStats, INT_MIN, INT_MAX, false, ""},
};

// the rule of `name` for `handle`, or nullptr: that handle has no such shared option
inline const OptionRule* find_option(const char* name, int handle)
{
    for (const OptionRule& r : kOptionRules)
        if ((r.handles & handle) && !strcmp(r.name, name)) return &r;
    return nullptr;
}

inline bool option_value_ok(const OptionRule& r, int value) { return (value >= r.lo && value <= r.hi) || (r.zero_too && value == 0); }
