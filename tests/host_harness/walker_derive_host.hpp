// walker_derive_host.hpp -- TEST HARNESS ONLY.
// The per-env walker2d model constants as the DEVICE keeps them: derived in fp64 from the (fp32) xi lengths and stored in the
// kernels' scalar type (planar_kernels.hpp: walker_derive_lane).  The host harnesses used to derive them in T itself, so their
// fp32 build carried an fp32 model derivation -- inertias, inverse weights -- that no kernel runs.
#pragma once
#include "../../random-envs_amd/csrc/planar_model.hpp"

template <class T>
static void walker_geom_like_device(const T* xi, rex::PlanarGeom<T, rex::Walker2dSpec>& G) {
  using S = rex::Walker2dSpec;
  rex::PlanarGeom<double, S> Gd; rex::SolParams<double> spd; double nominal[S::NB];
  const double len[4] = {double(xi[7]), double(xi[8]), double(xi[9]), double(xi[10])};
  rex::derive_model<double, S>(len, Gd, nominal, spd);
  const double* src = reinterpret_cast<const double*>(&Gd); T* dst = reinterpret_cast<T*>(&G);
  for (size_t k = 0; k < sizeof(Gd) / sizeof(double); k++) dst[k] = T(src[k]);
}
