// check_mean_cert_host.cpp -- csrc/knn_mean_cert.h on the host, as a program of its own (no Python, no device, no HIP):
//
//   c++ -std=c++17 -O2 -ffp-contract=off tools/check_mean_cert_host.cpp -o /tmp/check_mean_cert_host
//
// (under the host sanitizers: add -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer as for
// tools/check_dev_carve_host.cpp)
//
//   check_mean_cert_host --constants     prints EPS and the short-root bound it is built from, as C hexadecimal floats
//   check_mean_cert_host < sums > out    reads float64 sums S (native byte order, 8 bytes each) from standard input and
//                                        writes 8 bytes per sum: the bits of f = (float)(S / 16), then `certain` as a uint32
//
// tests/test_mean_cert_host.py drives it and checks every answer against exact rational arithmetic.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../3dgsconverter_amd/csrc/knn_mean_cert.h"

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--constants")) {
        printf("eps %a\nshort_root_bound %a\n", gsx::KnnMeanEps::value, gsx::KNN_SHORT_ROOT_BOUND);
        return 0;
    }
    std::vector<double> in(1 << 16);
    std::vector<uint32_t> out(2 * in.size());
    for (;;) {
        const size_t n = fread(in.data(), sizeof(double), in.size(), stdin);
        if (n == 0) break;
        for (size_t i = 0; i < n; ++i) {
            const gsx::MeanCert c = gsx::mean_cert16<gsx::KnnMeanEps>(in[i]);
            memcpy(&out[2 * i], &c.f, 4);
            out[2 * i + 1] = c.certain ? 1u : 0u;
        }
        if (fwrite(out.data(), 8, n, stdout) != n) return 1;
    }
    return ferror(stdin) ? 1 : 0;
}
