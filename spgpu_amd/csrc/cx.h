#pragma once
/* The complex element of the ABI.  No HIP header: numeric.hip.h gives it its device arithmetic, csr_host.h only names it. */
namespace spgpu {

template <typename R> struct Cx { R x, y; };
using cfloat = Cx<float>;
using cdouble = Cx<double>;

} // namespace spgpu
