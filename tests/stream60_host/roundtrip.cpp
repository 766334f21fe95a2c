// The bit arithmetic of the lossless 60-bit value stream (stan_amd/csrc/s60.h: the very file the kernels include) on
// the host, over the edge values of its range: built with -fsanitize=address,undefined by tests/test_stream60_host.py.
// Exit code 0 and "ok <n>" when every encodable value comes back bit for bit and every other value is refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../stan_amd/csrc/s60.h"

static uint64_t bits_of(double a) { uint64_t u; std::memcpy(&u, &a, 8); return u; }

int main() {
    std::vector<double> good = {0.0, -0.0, 1.0, -1.0, std::nextafter(1.0, 0.0), std::nextafter(2.0, 0.0), -std::nextafter(2.0, 0.0),
                                std::ldexp(1.0, -126), -std::ldexp(1.0, -126), std::nextafter(std::ldexp(1.0, -126), 1.0), 0.5, -0.75};
    uint64_t s = 0x9e3779b97f4a7c15ull;   // xorshift: full 52-bit mantissas, every exponent of the range, both signs
    for (int i = 0; i < 20000; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const uint64_t u = (s & 0x800fffffffffffffull) | ((uint64_t)(897 + (s >> 52) % 127) << 52);
        double a; std::memcpy(&a, &u, 8);
        good.push_back(a);
    }
    const double inf = std::numeric_limits<double>::infinity();
    const std::vector<double> bad = {2.0, -2.0, std::nextafter(std::ldexp(1.0, -126), 0.0), std::numeric_limits<double>::denorm_min(),
                                     -std::numeric_limits<double>::denorm_min(), std::ldexp(1.0, -1022), inf, -inf,
                                     std::numeric_limits<double>::quiet_NaN(), 1e300, 3.0, std::ldexp(1.0, -127)};
    int errors = 0;
    // nine at a time through the packing of the high parts, as a lane of the encoder and of the products sees them
    for (size_t i0 = 0; i0 < good.size(); i0 += 9) {
        uint32_t lo[9], hi[9] = {0}, w[8];
        for (int j = 0; j < 9; j++) {
            const double a = i0 + j < good.size() ? good[i0 + j] : 0.0;
            if (!s60_encode(bits_of(a), &lo[j], &hi[j])) { std::printf("refused: %a\n", a); errors++; }
            if (hi[j] >> 28) { std::printf("high part wider than 28 bits: %a\n", a); errors++; }
        }
        s60_pack_high(hi, w);
        for (int j = 0; j < 9; j++) {
            const double a = i0 + j < good.size() ? good[i0 + j] : 0.0;
            const uint64_t back = s60_decode(lo[j], s60_high(w, j));
            if (back != bits_of(a)) { std::printf("%a came back as bits %016llx\n", a, (unsigned long long)back); errors++; }
        }
    }
    for (double a : bad) {
        uint32_t lo, hi;
        if (s60_encode(bits_of(a), &lo, &hi)) { std::printf("not refused: %a\n", a); errors++; }
        if (s60_decode(lo, hi) != 0) { std::printf("a refused entry must travel as +0.0: %a\n", a); errors++; }
    }
    if (errors) return 1;
    std::printf("ok %zu\n", good.size() + bad.size());
    return 0;
}
