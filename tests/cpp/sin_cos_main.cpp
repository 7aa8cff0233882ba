// Stand-alone check of pose::sin_cos (csrc/pose_solve.h), built with -ffp-contract=off and
// -fsanitize=address,undefined by tests/test_sin_cos_host.py: against the host's libm on two million arguments from
// 7e-6 to about 500 rad it stays within 1 ulp wherever |sin| or |cos| is above 1e-3 and within 4e-16 absolute
// elsewhere; sin^2 + cos^2 = 1 within 4 eps; the quadrant edges, 1e5 and what is not finite behave.
#include <cmath>
#include <cstdio>

#include "pose_solve.h"

static double ulps(double got, double want) {
  const double a = std::fabs(want);
  return std::fabs(got - want) / (std::nextafter(a, 1e300) - a);
}

int main() {
  double worst = 0, worst_abs = 0, worst_unit = 0;
  for (int i = 1; i < 2000000; i++) {
    const double x = i * 7.3e-6 * (1 + (i % 97) * 0.37);
    double s, c;
    msf::pose::sin_cos(x, &s, &c);
    const double ws = std::sin(x), wc = std::cos(x);
    if (std::fabs(ws) > 1e-3 && ulps(s, ws) > worst) worst = ulps(s, ws);
    if (std::fabs(wc) > 1e-3 && ulps(c, wc) > worst) worst = ulps(c, wc);
    if (std::fabs(s - ws) > worst_abs) worst_abs = std::fabs(s - ws);
    if (std::fabs(c - wc) > worst_abs) worst_abs = std::fabs(c - wc);
    if (std::fabs(s * s + c * c - 1) > worst_unit) worst_unit = std::fabs(s * s + c * c - 1);
  }
  std::printf("worst %g ulp, %g absolute, |s^2 + c^2 - 1| %g\n", worst, worst_abs, worst_unit);
  if (!(worst <= 1 && worst_abs <= 4e-16 && worst_unit <= 4 * 2.220446049250313e-16)) return 1;
  const double edges[] = {0.0, 1e-5, 0.78539816339744828, 0.7853981633974484, 1.5707963267948966, 3.141592653589793,
                          4.71238898038469, 6.283185307179586, 1e5};
  for (double x : edges) {
    double s, c;
    msf::pose::sin_cos(x, &s, &c);
    if (!(std::fabs(s - std::sin(x)) <= 4e-16 && std::fabs(c - std::cos(x)) <= 4e-16)) {
      std::printf("FAILED at %.17g\n", x);
      return 1;
    }
  }
  double s, c;
  msf::pose::sin_cos(1e300, &s, &c);
  if (!(std::fabs(s) <= 1 && std::fabs(c) <= 1)) return 1;
  msf::pose::sin_cos(NAN, &s, &c);
  if (!(std::isnan(s) && std::isnan(c))) return 1;
  msf::pose::sin_cos(INFINITY, &s, &c);
  if (!(std::isnan(s) && std::isnan(c))) return 1;
  std::printf("sin_cos checks passed\n");
  return 0;
}
