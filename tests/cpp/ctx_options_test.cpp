// csrc/fic_ctx_options.h as a program of its own, built with the host compiler's address and undefined-behaviour sanitizers
// (tests/test_ctx_options.py): for every shared option name and every handle kind that knows it, both boundaries are accepted,
// one step outside on each side is refused, lsq_tau_widen takes 0 but nothing else below 8, a handle that does not know a name
// finds no rule, and neither does anyone for an unknown name.  The expectations below are written out here, not read from the table.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "../../fractal-image-compression_amd/csrc/fic_ctx_options.h"

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            failures++;                                   \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

struct Want {
    const char* name;
    int handles;         // who knows the name
    int lo, hi;
    bool ranged;         // false: a switch, every value is accepted
    const char* words;   // part of the refusal's text
};

static const Want kWant[] = {
    {"search", kOptGrey | kOptRgb | kOptQt, 0, 1, true, "0 (the reference's criterion) or 1 (least squares)"},
    {"chunks", kOptGrey | kOptRgb, 0, INT_MAX, true, ">= 0"},
    {"q_eshift", kOptGrey | kOptRgb, -12, 4, true, "-12..4"},
    {"lsq_tau_widen", kOptGrey | kOptRgb, 8, 24, true, "0 (off) or in 8..24"},
    {"lsq_engine", kOptGrey | kOptRgb, 0, 1, true, "matrix cores"},
    {"lsq_q_eshift", kOptGrey | kOptRgb, -12, 4, true, "-12..4"},
    {"time_sweep", kOptGrey | kOptRgb, 0, 0, false, ""},
    {"sweep_stats", kOptGrey | kOptRgb, 0, 0, false, ""},
};

int main()
{
    const int handles[3] = {kOptGrey, kOptRgb, kOptQt};
    const char* hname[3] = {"grey", "rgb", "qt"};
    for (const Want& w : kWant) {
        for (int i = 0; i < 3; i++) {
            const OptionRule* r = find_option(w.name, handles[i]);
            if (!(w.handles & handles[i])) {
                CHECK(r == nullptr, "%s handle knows '%s'", hname[i], w.name);
                continue;
            }
            CHECK(r != nullptr, "%s handle has no rule for '%s'", hname[i], w.name);
            if (!r) continue;
            CHECK(!strcmp(r->name, w.name) && (r->handles & handles[i]), "%s: rule '%s' of handles %d", w.name, r->name, r->handles);
            if (!w.ranged) {
                const int any[] = {INT_MIN, -1, 0, 1, 2, INT_MAX};
                for (int v : any) CHECK(option_value_ok(*r, v), "%s (%s): switch refuses %d", w.name, hname[i], v);
                continue;
            }
            CHECK(option_value_ok(*r, w.lo), "%s (%s): lowest value %d refused", w.name, hname[i], w.lo);
            CHECK(option_value_ok(*r, w.hi), "%s (%s): highest value %d refused", w.name, hname[i], w.hi);
            const bool gap = !strcmp(w.name, "lsq_tau_widen");
            if (w.lo > INT_MIN) CHECK(!option_value_ok(*r, w.lo - 1), "%s (%s): %d accepted", w.name, hname[i], w.lo - 1);
            if (w.hi < INT_MAX) CHECK(!option_value_ok(*r, w.hi + 1), "%s (%s): %d accepted", w.name, hname[i], w.hi + 1);
            CHECK(!option_value_ok(*r, INT_MIN), "%s (%s): INT_MIN accepted", w.name, hname[i]);
            if (gap) {
                CHECK(option_value_ok(*r, 0), "lsq_tau_widen (%s): 0 refused", hname[i]);
                CHECK(!option_value_ok(*r, 1) && !option_value_ok(*r, 7) && !option_value_ok(*r, -1), "lsq_tau_widen (%s): a value of the gap accepted", hname[i]);
            }
            CHECK(strstr(r->must, "must ") == r->must && strstr(r->must, w.words), "%s (%s): refusal reads '%s'", w.name, hname[i], r->must);
        }
    }
    // the two handles name their own kernels
    CHECK(strstr(find_option("lsq_engine", kOptGrey)->must, "k_sweep_lsq_q)"), "grey lsq_engine text");
    CHECK(strstr(find_option("lsq_engine", kOptRgb)->must, "k_sweep_lsq_rgb_q)"), "rgb lsq_engine text");
    const char* own[] = {"no_such_option", "", "sweep", "q_shape", "q_noflag", "Search", "search "};
    for (const char* n : own)
        for (int i = 0; i < 3; i++) CHECK(find_option(n, handles[i]) == nullptr, "%s handle finds a shared rule for '%s'", hname[i], n);
    // every row of the table is one somebody expects
    for (const OptionRule& r : kOptionRules) {
        bool known = false;
        for (const Want& w : kWant) known = known || (!strcmp(w.name, r.name) && (w.handles & r.handles) == r.handles);
        CHECK(known && r.handles != 0 && r.lo <= r.hi, "row '%s' (handles %d, %d..%d)", r.name, r.handles, r.lo, r.hi);
    }
    printf("%d checks\n%d failures\n", checks, failures);
    return failures ? 1 : 0;
}
