// In-place mixed-radix complex FFT on lines held in LDS, for lengths L = m 2^a, m in {1, 3, 5}, a >= 2, 4 <= L <= 1024 (tdr_freq_loss.hip).
//
// Forward: decimation in frequency (butterfly, then twiddle), natural order in, DIGIT-REVERSED order out.  With the radices r_0 .. r_{s-1}
// of the plan and pos = p_0 L/r_0 + p_1 L/(r_0 r_1) + ..., position pos holds frequency k = p_0 + r_0 (p_1 + r_1 (p_2 + ...)).
// Inverse: decimation in time over the same radices in reverse (conjugate twiddle, then conjugate butterfly), digit-reversed in, natural
// out, unnormalised.  A pointwise step between the two needs no reordering at all; where the natural order is needed, fft_pos_of /
// fft_freq_at give the place.  Every butterfly reads and writes the same R places, so a stage needs one barrier and no second buffer.
// The odd radix, when there is one, is the first forward stage (sub-length L: its R inputs lie L/R apart), then radix 4, then one radix 2
// when a is odd.  Twiddles come from a table tw[t] = exp(-2 pi i t / L), t < L, correctly rounded from double.
//
// The file compiles on the host too (a test harness defines TDR_FFT_HOST): one "thread" then runs every butterfly of a stage in turn.
#pragma once

#ifdef TDR_FFT_HOST
struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { float2 r; r.x = x; r.y = y; return r; }
#define TDR_FFT_DEV static inline
#define TDR_FFT_SYNC() do { } while (0)
#else
#define TDR_FFT_DEV __device__ __forceinline__
#define TDR_FFT_SYNC() __syncthreads()
#endif

namespace tdr_fft {

constexpr int MAX_STAGES = 6;
constexpr int MAX_LEN = 1024;

struct Plan { int L, ns; int r[MAX_STAGES]; };

// 1 for L = m 2^a with m in {1, 3, 5}, a >= 2, 4 <= L <= 1024
static inline int admissible(int L) {
    if (L < 4 || L > MAX_LEN) return 0;
    int a = 0;
    while ((L & 1) == 0) { L >>= 1; ++a; }
    return a >= 2 && (L == 1 || L == 3 || L == 5);
}

// split_tail: a closing radix-4 stage becomes two radix-2 stages (its four inputs are neighbouring elements: with 8 lines interleaved that
// is a 4-way LDS bank conflict for a 32-lane read group, where radix 2 is 2-way)
static inline Plan make_plan(int L, bool split_tail = false) {
    Plan p;
    p.L = L; p.ns = 0;
    for (int i = 0; i < MAX_STAGES; ++i) p.r[i] = 1;
    int rest = L;
    if (rest % 3 == 0) { p.r[p.ns++] = 3; rest /= 3; }
    if (rest % 5 == 0) { p.r[p.ns++] = 5; rest /= 5; }
    while (rest % 4 == 0) { p.r[p.ns++] = 4; rest /= 4; }
    if (rest == 2) p.r[p.ns++] = 2;
    if (split_tail && p.r[p.ns - 1] == 4) { p.r[p.ns - 1] = 2; p.r[p.ns++] = 2; }
    return p;
}

// the place that holds frequency k after the forward stages
TDR_FFT_DEV int fft_pos_of(const Plan& p, int k) {
    int pos = 0, sub = p.L;
    for (int s = 0; s < p.ns; ++s) {
        const int r = p.r[s];
        sub /= r;
        pos += (k % r) * sub;
        k /= r;
    }
    return pos;
}

// the frequency held at place pos after the forward stages
TDR_FFT_DEV int fft_freq_at(const Plan& p, int pos) {
    int k = 0, sub = p.L, mul = 1;
    for (int s = 0; s < p.ns; ++s) {
        const int r = p.r[s];
        sub /= r;
        const int d = pos / sub;
        pos -= d * sub;
        k += d * mul;
        mul *= r;
    }
    return k;
}

TDR_FFT_DEV float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
TDR_FFT_DEV float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
TDR_FFT_DEV float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
TDR_FFT_DEV float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
// -i a (forward) or +i a (inverse)
template <bool INV>
TDR_FFT_DEV float2 rot(float2 a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }

// y_p = sum_q x_q w^(p q), w = exp(-2 pi i / R), or its conjugate when INV
template <int R, bool INV>
TDR_FFT_DEV void butterfly(float2* x) {
    if (R == 2) {
        const float2 a = x[0], b = x[1];
        x[0] = cadd(a, b); x[1] = csub(a, b);
    } else if (R == 4) {
        const float2 t0 = cadd(x[0], x[2]), t1 = csub(x[0], x[2]), t2 = cadd(x[1], x[3]), t3 = rot<INV>(csub(x[1], x[3]));
        x[0] = cadd(t0, t2); x[2] = csub(t0, t2); x[1] = cadd(t1, t3); x[3] = csub(t1, t3);
    } else if (R == 3) {
        const float s = 0.86602540378443864676f;             // sin(2 pi / 3)
        const float2 t = cadd(x[1], x[2]), d = rot<INV>(csub(x[1], x[2]));
        const float2 m = make_float2(x[0].x - 0.5f * t.x, x[0].y - 0.5f * t.y);
        x[0] = cadd(x[0], t);
        x[1] = make_float2(m.x + s * d.x, m.y + s * d.y);
        x[2] = make_float2(m.x - s * d.x, m.y - s * d.y);
    } else {
        const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;     // cos(2 pi / 5), cos(4 pi / 5)
        const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;      // sin(2 pi / 5), sin(4 pi / 5)
        const float2 a1 = cadd(x[1], x[4]), a2 = cadd(x[2], x[3]), b1 = csub(x[1], x[4]), b2 = csub(x[2], x[3]);
        const float2 m1 = make_float2(x[0].x + c1 * a1.x + c2 * a2.x, x[0].y + c1 * a1.y + c2 * a2.y);
        const float2 m2 = make_float2(x[0].x + c2 * a1.x + c1 * a2.x, x[0].y + c2 * a1.y + c1 * a2.y);
        const float2 n1 = rot<INV>(make_float2(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y));
        const float2 n2 = rot<INV>(make_float2(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y));
        x[0] = make_float2(x[0].x + a1.x + a2.x, x[0].y + a1.y + a2.y);
        x[1] = cadd(m1, n1); x[4] = csub(m1, n1);
        x[2] = cadd(m2, n2); x[3] = csub(m2, n2);
    }
}

// A line that lies contiguous in LDS carries one spare element after every 32: element i sits at pad32(i), so the strided reads of the
// late stages (4 or 16 elements apart) spread over the banks instead of meeting on a few (at most 2-way where they were 4-way).
TDR_FFT_DEV int pad32(int i) { return i + (i >> 5); }
static inline int padded_len(int L) { return L + (L >> 5); }

// one stage of sub-length n over nl lines.  LINE_FAST: element i of line l at buf[l * pl + i * es], neighbouring threads take the same
// butterfly of neighbouring lines (lines interleaved in memory, es = nl); otherwise element i of line l at buf[l * pl + pad32(i)],
// neighbouring threads take neighbouring butterflies of one line (es unused, pl >= padded_len(L)).
template <int R, bool INV, bool LINE_FAST>
TDR_FFT_DEV void stage(float2* buf, int L, int nl, int pl, int es, int n, const float2* tw, int tid, int nt) {
    const int m = n / R, per = L / R, total = per * nl, tws = L / n;
    // no division by m: an odd radix is the first stage (n = L, one block), and below it n, m are powers of two; LINE_FAST: nl is one too
    const int msh = (R == 2 || R == 4) ? __builtin_ctz(m) : 0, lsh = LINE_FAST ? __builtin_ctz(nl) : 0;
    for (int id = tid; id < total; id += nt) {
        int l, u;
        if (LINE_FAST) { u = id >> lsh; l = id & (nl - 1); } else { l = id / per; u = id - l * per; }
        const int bi = (R == 2 || R == 4) ? u >> msh : 0, j = u - bi * m;
        float2* p = buf + l * pl;
        const int e0 = bi * n + j;
        int at[R];
#pragma unroll
        for (int q = 0; q < R; ++q) at[q] = LINE_FAST ? (e0 + q * m) * es : pad32(e0 + q * m);
        float2 x[R];
#pragma unroll
        for (int q = 0; q < R; ++q) x[q] = p[at[q]];
        if (INV) {
#pragma unroll
            for (int q = 1; q < R; ++q) x[q] = cmulc(x[q], tw[j * q * tws]);
        }
        butterfly<R, INV>(x);
        if (!INV) {
#pragma unroll
            for (int q = 1; q < R; ++q) x[q] = cmul(x[q], tw[j * q * tws]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) p[at[q]] = x[q];
    }
}

template <bool INV, bool LINE_FAST>
TDR_FFT_DEV void stage_r(int r, float2* buf, int L, int nl, int pl, int es, int n, const float2* tw, int tid, int nt) {
    switch (r) {
        case 2: stage<2, INV, LINE_FAST>(buf, L, nl, pl, es, n, tw, tid, nt); break;
        case 3: stage<3, INV, LINE_FAST>(buf, L, nl, pl, es, n, tw, tid, nt); break;
        case 4: stage<4, INV, LINE_FAST>(buf, L, nl, pl, es, n, tw, tid, nt); break;
        default: stage<5, INV, LINE_FAST>(buf, L, nl, pl, es, n, tw, tid, nt); break;
    }
}

// all stages, a barrier after each; the caller's data must be visible (a barrier) before the call
template <bool LINE_FAST>
TDR_FFT_DEV void forward(const Plan& p, float2* buf, int nl, int pl, int es, const float2* tw, int tid, int nt) {
    int n = p.L;
    for (int s = 0; s < p.ns; ++s) {
        stage_r<false, LINE_FAST>(p.r[s], buf, p.L, nl, pl, es, n, tw, tid, nt);
        TDR_FFT_SYNC();
        n /= p.r[s];
    }
}

template <bool LINE_FAST>
TDR_FFT_DEV void inverse(const Plan& p, float2* buf, int nl, int pl, int es, const float2* tw, int tid, int nt) {
    int n = 1;
    for (int s = p.ns - 1; s >= 0; --s) {
        n *= p.r[s];
        stage_r<true, LINE_FAST>(p.r[s], buf, p.L, nl, pl, es, n, tw, tid, nt);
        TDR_FFT_SYNC();
    }
}

// Two real lines a, b transformed as one complex line z = a + i b: from Zk = Z[k] and Zn = Z[(L - k) mod L] the spectra A[k], B[k]
TDR_FFT_DEV void split_pair(float2 zk, float2 zn, float2& a, float2& b) {
    a = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    b = make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x));
}

// the reverse for the inverse transform: Z[k] = A[k] + i B[k], Z[L - k] = conj(A[k]) + i conj(B[k]) (A, B Hermitian)
TDR_FFT_DEV void merge_pair(float2 a, float2 b, float2& zk, float2& zn) {
    zk = make_float2(a.x - b.y, a.y + b.x);
    zn = make_float2(a.x + b.y, b.x - a.y);
}

}  // namespace tdr_fft
