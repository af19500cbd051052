// Driver of tests/test_native_objective.py: the objective of the response sensitivities (csrc/pl_objective.h) on cases read
// from stdin, one per line:
//     r|c  kind  p  n  has_weight  y[n] (r) or y[2n] interleaved (c)  [weight[n]]
// and per case one line "J d[0] d[1] ..." with %.17g: d = c[n] (r) or g[2n] interleaved (c).
#include <cstdio>
#include <vector>

#include "../../pylatticedso_amd/csrc/pl_objective.h"

int main() {
  char type;
  int kind, n, has_weight;
  double p;
  while (std::scanf(" %c %d %lf %d %d", &type, &kind, &p, &n, &has_weight) == 5) {
    if ((type != 'r' && type != 'c') || n < 1) return 2;
    const int width = type == 'c' ? 2 : 1;
    std::vector<double> y((size_t)width * n), w((size_t)n), d((size_t)width * n);
    for (double &v : y)
      if (std::scanf("%lf", &v) != 1) return 2;
    if (has_weight)
      for (double &v : w)
        if (std::scanf("%lf", &v) != 1) return 2;
    const double *wp = has_weight ? w.data() : nullptr;
    const double J = type == 'c' ? objective_complex(n, y.data(), kind, p, wp, d.data())
                                 : objective_real(n, y.data(), kind, p, wp, d.data());
    std::printf("%.17g", J);
    for (double v : d) std::printf(" %.17g", v);
    std::printf("\n");
  }
  return 0;
}
