// Host build of the limb forms (fhe-ram_amd/csrc/limb_forms.hpp through limb_forms_eval.hpp): the text the kernels call,
// compiled by a plain C++ compiler with -ffp-contract=off.  tests/test_limb_forms.py builds it twice:
//   as a shared object, loaded with ctypes:  limb_forms_eval_host(form, n, in, out)
//   as a stand-alone program (-DLIMB_FORMS_MAIN, with the sanitizers): main reads the whole edge grid from the file the test
//   wrote (tests/_limb_reference.py grid_file_bytes), evaluates every form, compares with the expected integers in the file
//   and prints a digest of the outputs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "limb_forms_eval.hpp"

extern "C" int limb_forms_eval_host(int form, int n, const double* in, double* out) {
    for (long i = 0; i < n; i++)
        if (fk::limb_form_eval(form, in + i * fk::LF_IN, out + i * fk::LF_OUT) != 0) return -1;
    return 0;
}

#ifdef LIMB_FORMS_MAIN
int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s GRID_FILE\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t digest = 0, index = 0;   // sum over the outputs' bit patterns times (2 * index + 1), modulo 2^64
    long total = 0, wrong = 0;
    int forms = 0;
    int32_t head[4];
    while (std::fread(head, sizeof(int32_t), 4, f) == 4) {
        const int form = head[0], n = head[1], n_in = head[2], n_out = head[3];
        if (n <= 0 || n > (1 << 20) || n_in <= 0 || n_in > fk::LF_IN || n_out <= 0 || n_out > fk::LF_OUT) { std::fprintf(stderr, "bad header\n"); return 2; }
        std::vector<double> used((size_t)n * n_in), in((size_t)n * fk::LF_IN, 0.0), out((size_t)n * fk::LF_OUT, 0.0);
        std::vector<int64_t> expect((size_t)n * n_out);
        if (std::fread(used.data(), sizeof(double), used.size(), f) != used.size() || std::fread(expect.data(), sizeof(int64_t), expect.size(), f) != expect.size()) {
            std::fprintf(stderr, "short file\n");
            return 2;
        }
        for (long i = 0; i < n; i++)
            for (int q = 0; q < n_in; q++) in[i * fk::LF_IN + q] = used[i * n_in + q];
        if (limb_forms_eval_host(form, n, in.data(), out.data()) != 0) { std::fprintf(stderr, "unknown form %d\n", form); return 2; }
        for (long i = 0; i < n; i++)
            for (int q = 0; q < n_out; q++) {
                const double o = out[i * fk::LF_OUT + q];
                if (o != (double)expect[i * n_out + q]) {
                    if (wrong < 10) std::fprintf(stderr, "form %d coefficient %ld output %d: %.17g, expected %lld\n", form, i, q, o, (long long)expect[i * n_out + q]);
                    wrong++;
                }
            }
        for (size_t b = 0; b < out.size(); b++, index++) {
            uint64_t bits;
            std::memcpy(&bits, &out[b], sizeof bits);
            digest += bits * (2 * index + 1);
        }
        total += n;
        forms++;
    }
    std::fclose(f);
    std::printf("forms %d coefficients %ld wrong %ld digest %016llx\n", forms, total, wrong, (unsigned long long)digest);
    return wrong ? 1 : 0;
}
#endif
