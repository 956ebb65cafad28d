// mccnn_amd/csrc/grad_clip.h compiled for the host: the scalar half of the clipped optimiser step against a table of cases.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mccnn_amd/csrc tools/grad_clip_check.cpp -o grad_clip_check
//   ./grad_clip_check            exit status 0 and "ok <cases>" when every case agrees
// The expected values are formed here in double and rounded once where the rule is one float32 operation, so a contracted or
// reordered evaluation in the header would show.
#include "grad_clip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

using namespace mccnn;

static long cases = 0;

static void expect(float norm, float max_norm, float coef, int skipped_on, const char* what) {
    const float got = clip_coef(norm, max_norm);
    const int s1 = clip_skipped(norm, 1), s0 = clip_skipped(norm, 0);
    uint32_t a, b;
    __builtin_memcpy(&a, &got, 4);
    __builtin_memcpy(&b, &coef, 4);
    if (a != b || s1 != skipped_on || s0 != 0) {
        std::printf("MISMATCH %s: norm %.9g max_norm %.9g -> coef %.9g (want %.9g), skipped %d (want %d), with the switch off %d\n", what,
                    (double)norm, (double)max_norm, (double)got, (double)coef, s1, skipped_on, s0);
        std::exit(1);
    }
    ++cases;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    // max_norm = 0: no clipping, whatever the norm
    for (float n : {0.0f, 1e-30f, 1.0f, 3.5f, 1e30f, big, inf, nan}) expect(n, 0.0f, 1.0f, std::isfinite(n) ? 0 : 1, "max_norm 0");
    // norm = 0: the quotient max_norm / 1e-6 is above 1 for every max_norm the entry takes above 1e-6
    for (float m : {1e-3f, 1.0f, 1e30f, big}) expect(0.0f, m, 1.0f, 0, "norm 0");
    expect(0.0f, 1e-7f, (float)(1e-7f / (double)1e-6f), 0, "norm 0 under a max_norm below the epsilon");
    // norm < max_norm: exactly 1
    expect(1.0f, 2.0f, 1.0f, 0, "norm < max_norm");
    expect(0.999f, 1.0f, 1.0f, 0, "norm < max_norm");
    expect(tiny, 1.0f, 1.0f, 0, "norm < max_norm");
    expect(1e29f, 1e30f, 1.0f, 0, "norm < max_norm");
    expect(3.9999f, 4.0f, 1.0f, 0, "norm < max_norm");
    // norm > max_norm: float32(max_norm / float32(norm + 1e-6f))
    const float pairs[][2] = {{4.0f, 1.0f}, {3.0f, 1.0f}, {1.0f, 0.25f}, {123.456f, 7.0f}, {1e30f, 1.0f}, {big, 1.0f}, {1e-3f, 1e-4f},
                              {2.5e-6f, 1e-6f}, {1.0f, 1.0f},
                              {std::nextafterf(4.0f, 0.0f), 4.0f}};   // (the last: within the epsilon below max_norm still clips)
    for (const auto& p : pairs) {
        // (a sum or quotient of two floats formed in double and rounded to float is the correctly rounded float32 result:
        // 53 >= 2 * 24 + 2 bits make the double rounding harmless)
        const float den = (float)((double)p[0] + (double)1e-6f);
        const float want = (float)((double)p[1] / (double)den);
        if (!(want < 1.0f)) { std::printf("the case %g / %g does not clip\n", (double)p[1], (double)p[0]); return 2; }
        expect(p[0], p[1], want, 0, "norm > max_norm");
    }
    // norm inf and NaN: the coefficient stays 1, the skip flag follows its switch
    for (float m : {0.0f, 1e-3f, 1.0f, big}) {
        expect(inf, m, 1.0f, 1, "norm inf");
        expect(nan, m, 1.0f, 1, "norm NaN");
        expect(-nan, m, 1.0f, 1, "norm -NaN");
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
