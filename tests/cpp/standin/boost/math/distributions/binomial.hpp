// tests/cpp/standin/boost/math/distributions/binomial.hpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
// Stand-in for the one boost header the reference's MIBFQuerySupport.hpp includes: the type its `using` names and the
// cdf its calcSat calls.  calcSat has no caller, so cdf only has to compile.
#pragma once
namespace boost {
namespace math {
struct binomial
{
	binomial(double, double) {}
};
inline double cdf(const binomial&, double) { return 0.0; }
} // namespace math
} // namespace boost
