// Host-side argument checks the *_create functions of the frame-observable units share: "every index of a list is in
// [0, n)" and the site geometry + box of an oxDNA observable set.  They run in front of select_device, so a bad list is
// refused without a GPU.  Stands on <cstdint>, <string> and set_error alone (the host test of oracle/cpu_port compiles
// it as it is, like device_buf.h).
#ifndef MYTHOS_HOST_CHECKS_H
#define MYTHOS_HOST_CHECKS_H

#include <cstddef>
#include <cstdint>
#include <string>

namespace mythos {

void set_error(const std::string& msg);

// list[0 .. count) all in [0, n): true.  Otherwise false, with `what` as the error message.  count = 0 reads nothing
// (list may be null).
inline bool indices_in_range(const int32_t* list, size_t count, int n, const char* what) {
  for (size_t k = 0; k < count; ++k)
    if (list[k] < 0 || list[k] >= n) {
      set_error(what);
      return false;
    }
  return true;
}

// Where the sites of a nucleotide are and how displacements between them wrap: base site c + g_hb a1, backbone site
// c + g_k1 a1 + g_k2 a2 (model 3, oxRNA2: g_k2 a3; model 1 has no second coefficient).
struct SiteGeo {
  int model = 2;
  double g_hb = 0, g_k1 = 0, g_k2 = 0;
  int box_on = 0;
  double box[3] = {1, 1, 1};
};

// geometry: the three coefficients above; box: three edges, or null for free space.  false, with "<who>: ..." as the
// error message, for a box with an edge that is not positive (a NaN included).
inline bool site_geo_from(int model, const double* geometry, const double* box, const char* who, SiteGeo* g) {
  if (box && !(box[0] > 0 && box[1] > 0 && box[2] > 0)) {
    set_error(std::string(who) + ": box edges must be positive");
    return false;
  }
  g->model = model;
  g->g_hb = geometry[0], g->g_k1 = geometry[1], g->g_k2 = model >= 2 ? geometry[2] : 0.0;
  g->box_on = box ? 1 : 0;
  for (int k = 0; box && k < 3; ++k) g->box[k] = box[k];
  return true;
}

}  // namespace mythos

#endif  // MYTHOS_HOST_CHECKS_H
