// Host check of csrc/tdr_fft_core.h (compiled with TDR_FFT_HOST by tests/test_fft_core_host.py): every admissible length 4 ... 1024, both
// plans of make_plan (plain and split_tail), both line layouts (interleaved lines as the column pass holds them, padded lines as the row
// passes do), forward against a naive DFT in double, the digit-reversal functions against each other, forward + inverse = L x identity,
// and split_pair / merge_pair against the spectra of two real lines.  One "thread" runs every butterfly of a stage in turn.
#define TDR_FFT_HOST
#include "tdr_fft_core.h"
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace tdr_fft;
typedef std::complex<double> cd;

int main() {
    double worst = 0;
    int nadm = 0;
    for (int L = 1; L <= 1100; ++L) {
        if (!admissible(L)) continue;
        ++nadm;
      for (int tail = 0; tail < 2; ++tail) {
        Plan p = make_plan(L, tail == 1);
        int prod = 1;
        for (int s = 0; s < p.ns; ++s) prod *= p.r[s];
        if (prod != L || p.ns > MAX_STAGES) { printf("bad plan %d\n", L); return 1; }
        std::vector<float2> tw(L);
        for (int t = 0; t < L; ++t) tw[t] = make_float2((float)cos(-2.0 * M_PI * t / L), (float)sin(-2.0 * M_PI * t / L));
        // two lines interleaved (LINE_FAST, es = 2) and two padded lines one after the other (element i at pad32(i))
        for (int mode = 0; mode < 2; ++mode) {
            const int nl = 2;
            std::vector<float2> buf(nl * padded_len(L));
            std::vector<cd> ref(nl * L), in(nl * L);
            const int pl = mode ? 1 : padded_len(L), es = mode ? nl : 1;
            auto at = [&](int l, int i) { return mode ? l * pl + i * es : l * pl + pad32(i); };
            for (int l = 0; l < nl; ++l)
                for (int i = 0; i < L; ++i) {
                    float a = (float)rand() / RAND_MAX - 0.5f, b = (float)rand() / RAND_MAX - 0.5f;
                    buf[at(l, i)] = make_float2(a, b);
                    in[l * L + i] = cd(a, b);
                }
            for (int l = 0; l < nl; ++l)
                for (int k = 0; k < L; ++k) {
                    cd s = 0;
                    for (int i = 0; i < L; ++i) s += in[l * L + i] * std::polar(1.0, -2.0 * M_PI * ((long)k * i % L) / L);
                    ref[l * L + k] = s;
                }
            if (mode) forward<true>(p, buf.data(), nl, pl, es, tw.data(), 0, 1);
            else forward<false>(p, buf.data(), nl, pl, es, tw.data(), 0, 1);
            double e = 0, top = 0;
            for (int l = 0; l < nl; ++l)
                for (int k = 0; k < L; ++k) {
                    int pos = fft_pos_of(p, k);
                    if (fft_freq_at(p, pos) != k) { printf("rev mismatch L %d k %d\n", L, k); return 1; }
                    float2 v = buf[at(l, pos)];
                    e = fmax(e, std::abs(cd(v.x, v.y) - ref[l * L + k]));
                    top = fmax(top, std::abs(ref[l * L + k]));
                }
            if (mode) inverse<true>(p, buf.data(), nl, pl, es, tw.data(), 0, 1);
            else inverse<false>(p, buf.data(), nl, pl, es, tw.data(), 0, 1);
            double e2 = 0;
            for (int l = 0; l < nl; ++l)
                for (int i = 0; i < L; ++i) {
                    float2 v = buf[at(l, i)];
                    e2 = fmax(e2, std::abs(cd(v.x, v.y) / (double)L - in[l * L + i]));
                }
            worst = fmax(worst, fmax(e / top, e2));
            if (e / top > 1e-6 || e2 > 1e-6) { printf("L %d mode %d fwd %g inv %g\n", L, mode, e / top, e2); return 1; }
        }
      }
    }
    // split / merge
    {
        int L = 48; Plan p = make_plan(L);
        std::vector<cd> a(L), b(L), A(L), B(L), Z(L);
        for (int i = 0; i < L; ++i) { a[i] = (double)rand() / RAND_MAX; b[i] = (double)rand() / RAND_MAX; }
        for (int k = 0; k < L; ++k) {
            A[k] = B[k] = Z[k] = 0;
            for (int i = 0; i < L; ++i) {
                cd w = std::polar(1.0, -2.0 * M_PI * k * i / L);
                A[k] += a[i] * w; B[k] += b[i] * w; Z[k] += (a[i] + cd(0, 1) * b[i]) * w;
            }
        }
        double e = 0;
        for (int k = 0; k <= L / 2; ++k) {
            float2 zk = make_float2(Z[k].real(), Z[k].imag()), zn = make_float2(Z[(L - k) % L].real(), Z[(L - k) % L].imag()), fa, fb, z1, z2;
            split_pair(zk, zn, fa, fb);
            e = fmax(e, std::abs(cd(fa.x, fa.y) - A[k])); e = fmax(e, std::abs(cd(fb.x, fb.y) - B[k]));
            merge_pair(make_float2(A[k].real(), A[k].imag()), make_float2(B[k].real(), B[k].imag()), z1, z2);
            e = fmax(e, std::abs(cd(z1.x, z1.y) - Z[k])); e = fmax(e, std::abs(cd(z2.x, z2.y) - Z[(L - k) % L]));
        }
        printf("split/merge err %g\n", e);
        if (e > 1e-4) return 1;
    }
    printf("ok: %d admissible lengths, worst rel err %g\n", nadm, worst);
    return 0;
}
