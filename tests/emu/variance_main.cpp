// variance_main.cpp -- stand-alone driver of the var / std arithmetic (polars_amd/csrc/variance.hpp: merge, from_shifted, finalize -- the one body of var_kernel, of
// the finaliser of the fused aggregates and of ops::reduce_var), built with -fsanitize=address,undefined by the tests.
// (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// What it is checked against shares nothing with the merge formula: a two-pass variance in long double over the whole input.
//   (1) merge over random splits: the input is cut into random pieces (empty pieces included), every piece reduced as var_kernel's lanes do (sums about the piece's
//       first value, from_shifted, the mean kept relative to the input's first value), the pieces merged in a random tree; |m2 - two-pass| within the bound of
//       DESIGN.md 4.14 with D = the data's own range.  The same with a common offset of 1e15: the bound does not move, because no step of the pipeline ever sees
//       the offset.  (The two-pass sum runs over x - offset, which is exact: at 1e15 a mean is representable to 0.06 only, in long double to 5e-5, and a two-pass
//       sum about such a mean is off by n times the square of that.)
//   (2) an empty side is the identity, bit for bit, and merging two empty sides makes no NaN.
//   (3) finalize: null when n <= ddof (every n 0..6 against every ddof 0..8, and ddof = 255), the division otherwise, std = sqrt(var).
//   (4) the clamp: sums whose difference rounds below zero give 0, never a negative variance or a NaN square root.
//   (5) NaN / +-inf among the values give NaN (valid), through from_shifted, through merge and through finalize.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/variance.hpp"

using namespace plx::variance;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, double got, double want) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %.17g, want %.17g\n", what, got, want);
}
static bool same_bits(double a, double b) { return !memcmp(&a, &b, 8); }

// one piece as a lane of var_kernel reduces it: sums about its first value, the mean relative to `origin`
static Moments piece(const double* x, size_t n, double origin = 0.0) {
  double p = 0, s1 = 0, s2 = 0;
  for (size_t i = 0; i < n; i++) { if (i == 0) p = x[0]; const double d = x[i] - p; s1 += d; s2 += d * d; }
  Moments m;
  m.n = (double)n; m.mean = n ? (p - origin) + s1 / (double)n : 0.0; m.m2 = from_shifted((double)n, s1, s2);
  return m;
}
static long double two_pass_m2(const std::vector<double>& x) {
  if (x.empty()) return 0;
  long double s = 0;
  for (double v : x) s += v;
  const long double mean = s / x.size();
  long double m2 = 0;
  for (double v : x) m2 += ((long double)v - mean) * ((long double)v - mean);
  return m2;
}
static Moments merge_tree(std::vector<Moments> parts, std::mt19937_64& rng) {
  while (parts.size() > 1) {
    const size_t i = rng() % (parts.size() - 1);
    parts[i] = merge(parts[i], parts[i + 1]);
    parts.erase(parts.begin() + (long)i + 1);
  }
  return parts.empty() ? Moments{0, 0, 0} : parts[0];
}

int main() {
  std::mt19937_64 rng(20240611);
  const double eps = std::ldexp(1.0, -53);
  // (1)
  for (int trial = 0; trial < 400; trial++) {
    const size_t n = trial < 8 ? (size_t)trial : (size_t)(rng() % 5000);
    const double offset = (trial & 1) ? 1e15 : 0.0, scale = std::ldexp(1.0, (int)(rng() % 40) - 20);
    std::normal_distribution<double> nd(0.0, scale);
    std::vector<double> x(n);
    for (auto& v : x) v = offset + nd(rng);
    std::vector<Moments> parts;
    for (size_t at = 0; at < n || parts.empty();) {
      size_t len = (rng() % 4 == 0) ? 0 : (size_t)(rng() % 300);
      if (len > n - at) len = n - at;
      parts.push_back(piece(x.data() + at, len, n ? x[0] : 0.0));
      at += len;
      if (at >= n) break;
    }
    if (rng() % 2) parts.push_back(Moments{0, 0, 0});
    const Moments m = merge_tree(parts, rng);
    std::vector<double> y(x);
    for (auto& v : y) v -= offset;      // exact: |v - offset| is far below offset
    const long double ref = two_pass_m2(y);
    double mn = 0, mx = 0;
    for (size_t i = 0; i < n; i++) { if (i == 0 || x[i] < mn) mn = x[i]; if (i == 0 || x[i] > mx) mx = x[i]; }
    const double D = mx - mn;
    // the contract's bound on m2 = n * var: 8 n eps (sigma^2 + D^2) n
    const double bound = 8.0 * (double)n * eps * ((double)(ref / (n ? n : 1)) + D * D) * (double)n;
    expect(m.n == (double)n, "merge: n", m.n, (double)n);
    expect(std::fabs((double)((long double)m.m2 - ref)) <= bound, "merge: m2 against the two-pass sum", m.m2, (double)ref);
    expect(m.m2 >= 0.0, "merge: m2 >= 0", m.m2, 0.0);
  }
  // (2)
  {
    const Moments a{7.0, 3.25, 11.5}, e{0.0, 0.0, 0.0};
    const Moments l = merge(e, a), r = merge(a, e), z = merge(e, e);
    expect(same_bits(l.n, a.n) && same_bits(l.mean, a.mean) && same_bits(l.m2, a.m2), "merge(empty, a) == a", l.m2, a.m2);
    expect(same_bits(r.n, a.n) && same_bits(r.mean, a.mean) && same_bits(r.m2, a.m2), "merge(a, empty) == a", r.m2, a.m2);
    expect(z.n == 0.0 && z.mean == z.mean && z.m2 == z.m2, "merge(empty, empty) makes no NaN", z.mean, 0.0);
    const Moments en{0.0, std::nan(""), std::nan("")};      // whatever an empty side carries is never read
    const Moments q = merge(a, en);
    expect(same_bits(q.mean, a.mean) && same_bits(q.m2, a.m2), "merge(a, empty with NaN fields) == a", q.m2, a.m2);
  }
  // (3)
  for (int n = 0; n <= 6; n++) {
    for (int ddof : {0, 1, 2, 3, 4, 5, 6, 7, 8, 255}) {
      bool valid = true;
      const double m2 = 2.0 * n;
      const double v = finalize((double)n, m2, ddof, false, &valid);
      bool svalid = true;
      const double s = finalize((double)n, m2, ddof, true, &svalid);
      expect(valid == (n > ddof) && svalid == valid, "finalize: valid iff n > ddof", (double)valid, (double)(n > ddof));
      if (n > ddof) {
        expect(v == m2 / (double)(n - ddof), "finalize: var = m2 / (n - ddof)", v, m2 / (double)(n - ddof));
        expect(s == std::sqrt(v), "finalize: std = sqrt(var)", s, std::sqrt(v));
      } else expect(v == 0.0 && s == 0.0, "finalize: a null carries 0", v, 0.0);
    }
  }
  // (4)
  {
    // three equal values about pivot 0: s2 - s1^2 / n cancels to a rounding error of either sign
    int negatives = 0;
    for (int i = 0; i < 20000; i++) {
      const double x = std::uniform_real_distribution<double>(0.1, 10.0)(rng);
      const double n = 3.0 + (double)(rng() % 5);
      double s1 = 0, s2 = 0;
      for (int j = 0; j < (int)n; j++) { s1 += x; s2 += x * x; }
      if (s2 - s1 * (s1 / n) < 0.0) negatives++;
      const double m2 = from_shifted(n, s1, s2);
      bool valid = false;
      const double sd = finalize(n, m2, 1, true, &valid);
      expect(m2 >= 0.0 && valid && sd >= 0.0 && sd == sd, "clamp: a constant group", m2, 0.0);
    }
    expect(negatives > 0, "clamp: the test data reach the clamp", (double)negatives, 1.0);
    expect(from_shifted(0.0, 0.0, 0.0) == 0.0, "from_shifted(0 rows)", from_shifted(0.0, 0.0, 0.0), 0.0);
    bool valid = false;
    expect(finalize(4.0, -1e-30, 0, true, &valid) == 0.0 && valid, "finalize: a negative m2 is 0", finalize(4.0, -1e-30, 0, true, &valid), 0.0);
  }
  // (5)
  {
    const double inf = INFINITY, nan = std::nan("");
    for (double special : {nan, inf, -inf}) {
      for (int pos = 0; pos < 3; pos++) {
        std::vector<double> x = {1.0, 2.0, 4.0, 8.0};
        x[pos] = special;
        for (double pivot : {0.0, 3.0}) {
          double s1 = 0, s2 = 0;
          for (double v : x) { s1 += v - pivot; s2 += (v - pivot) * (v - pivot); }
          bool valid = false;
          const double v = finalize(4.0, from_shifted(4.0, s1, s2), 1, false, &valid);
          expect(valid && v != v, "shifted sums with a NaN / inf value give NaN", v, nan);
        }
        const Moments m = merge(piece(x.data(), 2), piece(x.data() + 2, 2));
        bool valid = false;
        const double v = finalize(m.n, m.m2, 1, true, &valid);
        expect(valid && v != v, "merge with a NaN / inf value gives NaN", v, nan);
        const Moments m1 = merge(merge(piece(x.data(), 1), piece(x.data() + 1, 1)), merge(piece(x.data() + 2, 1), piece(x.data() + 3, 1)));
        const double v1 = finalize(m1.n, m1.m2, 0, false, &valid);
        expect(valid && v1 != v1, "merge of single rows with a NaN / inf value gives NaN", v1, nan);
      }
    }
    bool valid = true;
    const double one_inf = finalize(1.0, piece(&inf, 1).m2, 0, false, &valid);
    expect(valid && one_inf != one_inf, "one infinite row, ddof 0: NaN", one_inf, nan);
  }
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
