// wrap_idx (csrc/vx_sample.h), its rare block: the form that takes 1/n by mirroring the
// exponent of fn = (float)n (0x7F000000 - bits) and multiplies by fn, against the form it
// replaced (1.0f / (float)n and (float)n from the integer).  Host arithmetic only (IEEE
// fp32, no contraction): the two forms differ in how 1/n and (float)n are made, not in
// the operations on them.  Every noise side n = 2^k the API admits (k = 0..27), and for
// each: both signs of every exponent 24..62 with 4096 mantissas spread over the range
// and the 64 lowest and highest ones; the same below 2^24 (exponents -2..23: the kernel's
// fast path answers there and the block is not entered; the integer-valued ones also
// check the block's form against the fast path's mask, for n <= 2^24); +-0, +-inf and NaNs.
// Prints the number of values compared and of mismatches; exits 1 on any.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ivec(float) of the contract (vx_math.h f2i): NaN -> 0, saturate at +-2^24
static int f2i(float x) {
    const float c = std::fmin(std::fmax(x, -16777216.0f), 16777216.0f);
    return x == x ? (int)c : 0;
}

static int rare_old(float fl, int n) {
    const float q = std::floor(fl * (1.0f / (float)n));
    return f2i(fl - q * (float)n) & (n - 1);
}

static int rare_new(float fl, int n, float fn) {
    const float rn = u2f(0x7F000000u - f2u(fn));
    const float q = std::floor(fl * rn);
    return f2i(fl - q * fn) & (n - 1);
}

int main() {
    unsigned long long total = 0, bad = 0, fast_bad = 0;
    for (int k = 0; k <= 27; k++) {
        const int n = 1 << k;
        const float fn = (float)n;
        if (u2f(0x7F000000u - f2u(fn)) != 1.0f / fn || fn != std::ldexp(1.0f, k)) {
            std::printf("n = 2^%d: mirrored exponent is not 1/n\n", k);
            bad++;
        }
        auto one = [&](float fl) {
            total++;
            const int a = rare_old(fl, n), b = rare_new(fl, n, fn);
            if (a != b) {
                if (bad < 10) std::printf("n = 2^%d fl = %a: old %d new %d\n", k, fl, a, b);
                bad++;
            }
            // where the kernel's fast path answers, the rare form agrees with it for an integer-valued fl
            // (n <= 2^24: for a larger n the sum fl + n of a negative fl does not fit 24 bits, in
            // either form; the kernel never enters the block with |fl| < 2^24)
            if (k <= 24 && std::fabs(fl) < 16777216.0f && fl == std::floor(fl) && ((int)fl & (n - 1)) != b) fast_bad++;
        };
        for (int e = -2; e <= 62; e++) {
            for (uint32_t s = 0; s < 2; s++) {
                const uint32_t base = (s << 31) | ((uint32_t)(e + 127) << 23);
                for (uint32_t m = 0; m < 64; m++) { one(u2f(base | m)); one(u2f(base | (0x7FFFFFu - m))); }
                for (uint32_t j = 0; j < 4096; j++) one(u2f(base | ((j * 2047u + 977u * (uint32_t)k) & 0x7FFFFFu)));
                // integer-valued floats below 2^24 (the kernel passes floor(u))
                if (e >= 0 && e < 24)
                    for (uint32_t j = 0; j < 4096; j++) one(std::floor(u2f(base | ((j * 2053u) & 0x7FFFFFu))));
            }
        }
        const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u,
                                    0x7F800001u, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x00000001u, 0x80000001u};
        for (uint32_t u : special) one(u2f(u));
    }
    std::printf("wrap_idx rare block, old against new: %llu values over n = 2^0 .. 2^27, %llu mismatches; "
                "%llu disagreements with the fast path below 2^24 (n <= 2^24)\n", total, bad, fast_bad);
    return bad || fast_bad ? 1 : 0;
}
