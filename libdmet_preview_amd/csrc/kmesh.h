// Integer bookkeeping of a Gamma-centred k mesh in np.fft order (host only): shared by the mesh tables, folds and ERI plan of capi.hip
// and by the ERI pipeline (eri_engine.hip).
#pragma once
#include <vector>

struct Mesh {
    int n[3];
    int nk;
    explicit Mesh(const int m[3]) { n[0] = m[0]; n[1] = m[1]; n[2] = m[2]; nk = m[0] * m[1] * m[2]; }
    bool ok() const { return n[0] > 0 && n[1] > 0 && n[2] > 0 && (long long)n[0] * n[1] * n[2] < (1LL << 24); }
    void ints(int idx, int a[3]) const {
        a[2] = idx % n[2];
        a[1] = (idx / n[2]) % n[1];
        a[0] = idx / (n[2] * n[1]);
    }
    int index(const int a[3]) const { return (a[0] * n[1] + a[1]) * n[2] + a[2]; }
    static int mod(int x, int m) { int r = x % m; return r < 0 ? r + m : r; }
    int combine(int i, int j, int sign) const {   // idx(a_i + sign*a_j)
        int a[3], b[3], c[3];
        ints(i, a); ints(j, b);
        for (int d = 0; d < 3; ++d) c[d] = mod(a[d] + sign * b[d], n[d]);
        return index(c);
    }
    int minus(int i) const {
        int a[3], c[3];
        ints(i, a);
        for (int d = 0; d < 3; ++d) c[d] = mod(-a[d], n[d]);
        return index(c);
    }
    // fftfreq integer of mesh index a on an axis of length n
    static int freq(int a, int n) { return a <= (n - 1) / 2 ? a : a - n; }
};

// time-reversal weight of every k point: 1 for its own partner, 2 for the first of a pair (k, -k), 0 for the second
inline void tr_weights(const Mesh &m, int tr, std::vector<int> &w) {
    w.assign(m.nk, 1);
    if (!tr) return;
    for (int i = 0; i < m.nk; ++i) {
        const int mi = m.minus(i);
        w[i] = (mi == i) ? 1 : (mi > i ? 2 : 0);
    }
}
