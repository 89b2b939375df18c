// The one-shot quadtree entries run on the plan of ONE plane (csrc/fic_qt_batch_plan.h), so that plan must take
// every image they take.  A program of its own, built like qt_batch_plan_test.cpp under the host compiler's address and
// undefined-behaviour sanitizers (tests/test_qt_oneshot_plan.py), and with that program's check_plan: per ladder 16 -> 8,
// 16 -> 4 and 8 -> 4, the tallest image of the narrowest and of two square-ish widths that passes the size rules of the level
// geometries (qt_levels: fewer than 2^31 - 1 pixels, fewer than (2^31 - 1) / 8 domain blocks at every level), at the leaf
// widths 7, 8 and 9.
#define main qt_batch_plan_test_main        // that program's own cases: run by its own test
#include "qt_batch_plan_test.cpp"
#undef main

int main()
{
    int plans = 0;
    for (const Geo& ladder : {Geo{0, 0, 16, 8}, Geo{0, 0, 16, 4}, Geo{0, 0, 8, 4}})
        for (int w : {2 * ladder.B_max, 32768, 46336}) {
            auto taken = [&](long long h) {
                const long long Dw = 2 * (w / ladder.B_min) - 3, Dh = 2 * (h / ladder.B_min) - 3;
                return (long long)w * h < 0x7FFFFFFFll && Dw * Dh * 8 < 0x7FFFFFFFll;
            };
            long long h = 0x7FFFFFFFll / w / ladder.B_max * ladder.B_max;
            while (h > 0 && !taken(h)) h -= ladder.B_max;
            CHECK(h >= 2 * ladder.B_max && !taken(h + ladder.B_max), "%d -> %d, width %d: no tallest image", ladder.B_max, ladder.B_min, w);
            for (int leaf_ints : {7, 8, 9}) {
                check_plan(Geo{w, (int)h, ladder.B_max, ladder.B_min}, 1, leaf_ints);
                plans++;
            }
        }
    printf("%d one-plane plans at the largest images checked\n%d failures\n", plans, failures);
    return failures ? 1 : 0;
}
