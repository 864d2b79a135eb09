// Sanitizer target of the CPU port (TEST INFRASTRUCTURE): reads a system written by tests/test_cpu_port.py, evaluates
// energies and forces, runs a few Langevin steps with list rebuilds, prints the numbers.  Built twice by
// oracle/Makefile: plain, and with -fsanitize=address,undefined (the test compares the two outputs and requires a
// clean sanitizer log).  File layout: int32 {model, n, n_bonded, n_params, has_box, n_steps}, then seq int32[n],
// is_end int32[n], bonded int32[n_bonded][2], box double[3], flat double[n_params], center double[n][3], quat double[n][4],
// and for model 4 (oxNA; n_params = three vectors) is_rna int32[n].
// MARTINI (martini_cpu.cpp, which instantiates mythos_amd/csrc/martini_terms.h): int32 {10, n, n_bonds, n_angles, n_types,
// n_steps}, then types int32[n], bonds int32[n_bonds][2], angles int32[n_angles][3], box double[3], sigma and eps
// double[n_types][n_types], bond k and r0 double[n_bonds], angle k and theta0 double[n_angles], mass, x and v double[n](,[3]);
// evaluated and stepped once with G96 and once with harmonic angles.
// `--device-buf` instead of a file: the owning buffer types of the library (mythos_amd/csrc/device_buf.h: DeviceBuf, and
// PinnedBuf for pinned host memory) over the shim's malloc-backed runtime; prints what was read back and, after every
// scope, the live allocations (the test wants 0).
// `--md-plan`: the launch plan of the oxDNA step kernel (mythos_amd/csrc/md_plan.h) for a fixed table of systems, one line
// each: lanes per nucleotide, then nucleotides per workgroup, workgroups, grid, the DENSE choice and the priority switch.
// `--index-lists`: the argument checks the *_create functions of the frame observables share (mythos_amd/csrc/host_checks.h):
// empty lists, the last valid and the first invalid index on either side, boxes with an edge that is not positive; one
// line per case with the verdict and the error message it left.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "device_buf.h"
#include "host_checks.h"
#include "md_plan.h"

namespace mythos {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
int hip_fail(hipError_t e, const char* what) {
  g_error = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
  return MYTHOS_ERR_HIP;
}
}  // namespace mythos

extern "C" {
void* mythos_cpu_create(int model, int n, const int32_t* seq, const uint8_t* is_end, int n_bonded, const int32_t* bonded,
                        const double* box, const double* flat, int n_params);
void mythos_cpu_destroy(void* h);
void mythos_cpu_set_types(void* h, const uint8_t* is_rna);
int mythos_cpu_build_pairs(void* h, const double* center, double r_list);
int mythos_cpu_energy(void* h, const double* center, const double* quat, double* e_terms, double* dU_dcenter,
                      double* dU_dquat, double* torque_body);
int mythos_cpu_langevin_run(void* h, double* c, double* q, double* p, double* L, int n_steps, double dt, double kT,
                            double gamma_t, double gamma_r, double mass, const double* inertia, uint64_t seed,
                            int64_t step0, double r_cut, double skin, int rebuild_every, double* e_last);
void* mythos_cpu_martini_create(int n, const int32_t* types, int n_types, const double* sigma, const double* eps, int n_bonds,
                                const int32_t* bonds, const double* bk, const double* br0, int n_angles, const int32_t* angles,
                                const double* ak, const double* at0, int angle_kind, double r_cut, const double* mass);
void mythos_cpu_martini_destroy(void* h);
void mythos_cpu_martini_energy(void* h, const double* x, const double* box, double* e3, double* g);
int mythos_cpu_martini_run(void* h, double* x, double* v, const double* box, int n_steps, double dt, double kT, double gamma,
                           uint64_t seed, int64_t step0, double skin, int rebuild_every, double* e4);
}

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

static int martini_case(FILE* f, int n, int nb, int na, int nt, int n_steps) {
  const auto types = rd<int32_t>(f, n);
  const auto bonds = rd<int32_t>(f, 2 * (size_t)nb);
  const auto angles = rd<int32_t>(f, 3 * (size_t)na);
  const auto box = rd<double>(f, 3);
  const auto sigma = rd<double>(f, (size_t)nt * nt), eps = rd<double>(f, (size_t)nt * nt);
  const auto bk = rd<double>(f, nb), br0 = rd<double>(f, nb), ak = rd<double>(f, na), at0 = rd<double>(f, na);
  const auto mass = rd<double>(f, n), x0 = rd<double>(f, 3 * (size_t)n), v0 = rd<double>(f, 3 * (size_t)n);
  fclose(f);
  for (int kind = 0; kind < 2; ++kind) {
    void* h = mythos_cpu_martini_create(n, types.data(), nt, sigma.data(), eps.data(), nb, bonds.data(), bk.data(), br0.data(), na,
                                        angles.data(), ak.data(), at0.data(), kind, 1.1, mass.data());
    if (!h) return 3;
    auto x = x0, v = v0;
    double e[4];
    std::vector<double> g(3 * (size_t)n);
    mythos_cpu_martini_energy(h, x.data(), box.data(), e, g.data());
    printf("E %.12e %.12e %.12e", e[0], e[1], e[2]);
    double fs[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) fs[k] += g[3 * (size_t)i + k];
    printf("\nFSUM %.3e %.3e %.3e\n", fs[0], fs[1], fs[2]);
    const int builds = mythos_cpu_martini_run(h, x.data(), v.data(), box.data(), n_steps, 0.02, 2.27, 1.0, 42, 0, 0.2, 3, e);
    printf("MD builds %d E %.10e %.10e %.10e %.10e", builds, e[0], e[1], e[2], e[3]);
    printf("\nX %.12e %.12e %.12e\n", x[0], x[3 * (size_t)(n - 1) + 2], v[3 * (size_t)(n / 2)]);
    mythos_cpu_martini_destroy(h);
  }
  return 0;
}

static void live(const char* scope) { printf("DEVBUF %s live %ld\n", scope, shim_live_allocations()); }

struct FourBuffers {
  mythos::DeviceBuf<int> a, b;
  mythos::DeviceBytes c;
  mythos::DeviceBuf<double> d;
  int create() {  // as a *_create of the library: the first failure ends it, the destructor cleans up
    if (int rc = a.alloc(8)) return rc;
    if (int rc = b.alloc(8)) return rc;
    if (int rc = c.alloc(64)) return rc;
    return d.alloc(8);
  }
};

struct PinnedAndDevice {
  mythos::DeviceBuf<int> a;
  mythos::PinnedBuf<int> p, q;
  int create() {
    if (int rc = a.alloc(8)) return rc;
    if (int rc = p.alloc(8)) return rc;
    return q.alloc(8);
  }
};

// the ownership rules of DeviceBuf again for PinnedBuf: 0, or the code of the first check that failed
static int pinned_buf_checks() {
  using mythos::PinnedBuf;
  {
    PinnedBuf<double> g;
    if (g.grow(0) || g.host() != nullptr || g) return 70;  // nothing needed, nothing allocated
    if (g.grow(16) || !g.host() || g.dev() != g.host()) return 71;  // (the shim's device reads at the host's address)
    const double* p0 = g.host();
    if (g.grow(16) || g.grow(7) || g.host() != p0 || g.capacity() != 16) return 72;
    if (g.grow(17) || g.capacity() != 17) return 73;
    memset(g.host(), 0, 17 * sizeof(double));  // (the sanitizer build checks the extent)
    if (g.alloc(0) || !g.host() || g.capacity() != 1) return 74;  // never a zero-byte allocation
    printf("PINNED grow cap %zu held %ld\n", g.capacity(), shim_live_allocations());
  }
  if (shim_live_allocations() != 0) return 75;
  {
    PinnedBuf<int> a;
    if (a.alloc(4)) return 80;
    int *pa = a.host(), *da = a.dev();
    PinnedBuf<int> b(std::move(a));
    if (a.host() != nullptr || a.dev() != nullptr || a.capacity() != 0 || b.host() != pa || b.dev() != da || b.capacity() != 4) return 81;
    PinnedBuf<int> c;
    if (c.alloc(2)) return 82;
    c = std::move(b);  // frees c's own allocation
    if (b.host() != nullptr || c.host() != pa || c.capacity() != 4) return 83;
    printf("PINNED moved held %ld\n", shim_live_allocations());
    c.reset();
    if (c.host() != nullptr || c.dev() != nullptr || c.capacity() != 0 || c) return 84;
    c.reset();  // twice: nothing to do
    printf("PINNED reset held %ld\n", shim_live_allocations());
  }
  if (shim_live_allocations() != 0) return 85;
  {
    PinnedAndDevice h;
    shim_fail_allocation_in() = 3;
    const int rc = h.create();
    printf("PINNED partial rc %d a %d p %d q %d held %ld: %s\n", rc, h.a ? 1 : 0, h.p ? 1 : 0, h.q ? 1 : 0, shim_live_allocations(),
           mythos::g_error.c_str());
    if (rc != MYTHOS_ERR_HIP || !h.p || h.q || h.q.dev() || h.q.capacity() != 0) return 90;
  }
  return shim_live_allocations() == 0 ? 0 : 91;
}

static int device_buf_case() {
  using mythos::DeviceBuf;
  using mythos::DeviceBytes;
  {
    DeviceBuf<int> b;
    const std::vector<int> v = {3, 1, 4, 1, 5, 9, 2, 6};
    int back[8] = {};
    if (b.alloc(5) || b.capacity() != 5 || b.upload(v) || b.capacity() != 8) return 10;
    hipMemcpy(back, b.get(), sizeof(back), hipMemcpyDeviceToHost);
    printf("DEVBUF upload %d %d %d cap %zu\n", back[0], back[4], back[7], b.capacity());
    if (b.upload(v.data(), 3) || b.capacity() != 3) return 11;
    hipMemcpy(back, b.get(), 3 * sizeof(int), hipMemcpyDeviceToHost);
    printf("DEVBUF upload3 %d %d cap %zu\n", back[0], back[2], b.capacity());
  }
  live("upload");
  {
    DeviceBuf<double> g;
    if (g.grow(0) || g.get() != nullptr) return 20;  // nothing needed, nothing allocated
    if (g.grow(16)) return 21;
    const double* p0 = g.get();
    if (g.grow(16) || g.grow(7) || g.get() != p0 || g.capacity() != 16) return 22;  // at or below capacity: untouched
    if (g.grow(17) || g.capacity() != 17) return 23;
    hipMemset(g.get(), 0, 17 * sizeof(double));  // (the sanitizer build checks the extent)
    printf("DEVBUF grow cap %zu held %ld\n", g.capacity(), shim_live_allocations());
  }
  live("grow");
  {
    DeviceBuf<int> a;
    if (a.alloc(4)) return 30;
    int* pa = a.get();
    DeviceBuf<int> b(std::move(a));
    if (a.get() != nullptr || a.capacity() != 0 || b.get() != pa || b.capacity() != 4) return 31;
    DeviceBuf<int> c;
    if (c.alloc(2)) return 32;
    c = std::move(b);  // frees c's own allocation
    if (b.get() != nullptr || c.get() != pa || c.capacity() != 4) return 33;
    printf("DEVBUF moved held %ld\n", shim_live_allocations());
    c.reset();
    if (c.get() != nullptr || c.capacity() != 0 || c) return 34;
    c.reset();  // twice: nothing to do
    printf("DEVBUF reset held %ld\n", shim_live_allocations());
  }
  live("move");
  {
    DeviceBuf<int> z;
    DeviceBytes r;
    if (z.alloc(0) || !z.get() || z.capacity() != 1) return 40;  // never a zero-byte allocation
    if (z.upload(nullptr, 0) || !z.get() || z.capacity() != 1) return 41;
    if (r.upload_real(MYTHOS_F32, nullptr, 0) || !r.get() || r.capacity() != 1) return 42;
    const double src[3] = {0.1, 2.0, -1.0 / 3.0};
    float f[3];
    double d[3];
    if (r.upload_real(MYTHOS_F32, src, 3) || r.capacity() != 3 * sizeof(float)) return 43;
    hipMemcpy(f, r.get(), sizeof(f), hipMemcpyDeviceToHost);
    if (r.upload_real(MYTHOS_F64, src, 3) || r.capacity() != 3 * sizeof(double)) return 44;
    hipMemcpy(d, r.get(), sizeof(d), hipMemcpyDeviceToHost);
    printf("DEVBUF real %.9e %.9e %.17e %.17e\n", (double)f[0], (double)f[2], d[0], d[2]);
    if (f[0] != float(src[0]) || f[2] != float(src[2]) || memcmp(d, src, sizeof(d)) != 0) return 45;
  }
  live("zero");
  {
    FourBuffers h;
    shim_fail_allocation_in() = 3;
    const int rc = h.create();
    printf("DEVBUF partial rc %d a %d b %d c %d d %d held %ld: %s\n", rc, h.a ? 1 : 0, h.b ? 1 : 0, h.c ? 1 : 0, h.d ? 1 : 0,
           shim_live_allocations(), mythos::g_error.c_str());
    if (rc != MYTHOS_ERR_HIP || h.c || h.d) return 50;
  }
  live("partial");
  if (int rc = pinned_buf_checks()) return rc;
  {
    const int ok = mythos::select_device(0, "selftest"), bad = mythos::select_device(3, "selftest");
    printf("DEVBUF select %d %d: %s\n", ok, bad, mythos::g_error.c_str());
  }
  return shim_live_allocations() == 0 ? 0 : 60;
}

// md_plan.h at the sizes where a choice changes (the thresholds are in workgroups per CU, so they move with `cus`)
static int md_plan_case() {
  struct Row {
    int n, cus, real_bytes, debug_lanes, debug_dense;
  };
  const Row rows[] = {
      // lanes: 16 up to 6 144 nt on 256 CUs, the override wins at either size
      {6144, 256, 4, 0, 0}, {6145, 256, 4, 0, 0}, {6144, 256, 4, 8, 0}, {6145, 256, 4, 16, 0}, {64, 256, 4, 0, 0},
      // DENSE: fp32, 8 lanes, more than four workgroups per CU; forced and forbidden; never fp64, never 16 lanes
      {32768, 256, 4, 0, 0}, {32769, 256, 4, 0, 0}, {32769, 256, 8, 0, 0}, {64, 256, 4, 8, 1}, {32769, 256, 4, 0, 2},
      {64, 256, 4, 16, 1}, {32769, 256, 4, 16, 0}, {32769, 256, 8, 0, 1},
      // priority: off for fp64 grids of more than three workgroups per CU
      {24000, 256, 8, 0, 0}, {24577, 256, 8, 0, 0}, {24577, 256, 4, 0, 0},
      // another device: 304 CUs move every threshold
      {6145, 304, 4, 0, 0}, {7296, 304, 4, 0, 0}, {7297, 304, 4, 0, 0}, {32769, 304, 4, 0, 0}, {38913, 304, 4, 0, 0},
      {24577, 304, 8, 0, 0}, {29185, 304, 8, 0, 0},
  };
  for (const Row& r : rows) {
    const int lanes = mythos::md_lanes_for(r.n, r.cus, r.debug_lanes);
    const mythos::MdPlan p = mythos::md_plan_for(r.n, lanes, r.cus, (size_t)r.real_bytes, r.debug_dense);
    printf("MDPLAN n %d cus %d fp%d dbg_lanes %d dbg_dense %d -> lanes %d ppb %d blocks %d grid %d dense %d prio %d\n", r.n, r.cus,
           8 * r.real_bytes, r.debug_lanes, r.debug_dense, lanes, p.ppb, p.blocks, p.grid, p.dense_grid ? 1 : 0, p.prio_on);
  }
  return 0;
}

// host_checks.h on lists of exactly the length they are said to have (the sanitizer build sees a read past either end)
static int index_lists_case() {
  using mythos::indices_in_range;
  auto list_case = [](const char* name, const std::vector<int32_t>& v, int n) {
    const std::vector<int32_t> exact(v);  // capacity == size
    mythos::g_error = "-";
    const bool ok = indices_in_range(exact.data(), exact.size(), n, name);
    printf("LISTS %s count %zu n %d -> %d: %s\n", name, exact.size(), n, ok ? 1 : 0, mythos::g_error.c_str());
    return ok;
  };
  mythos::g_error = "-";
  const bool null_ok = indices_in_range(nullptr, 0, 5, "null");
  printf("LISTS null count 0 n 5 -> %d: %s\n", null_ok ? 1 : 0, mythos::g_error.c_str());
  if (!null_ok || !list_case("empty", {}, 5)) return 70;
  if (!list_case("first-and-last-valid", {0, 4, 2, 4}, 5) || !list_case("one-nucleotide", {0}, 1)) return 71;
  if (list_case("n-itself", {0, 4, 5}, 5) || list_case("minus-one", {0, -1, 4}, 5) || list_case("n-at-the-front", {5, 0}, 5) ||
      list_case("minus-one-at-the-end", {3, 2, 1, 0, -1}, 5) || list_case("int-min", {INT32_MIN}, 5) || list_case("int-max", {INT32_MAX}, INT32_MAX))
    return 72;
  const double geometry[3] = {0.4, -0.4, 0.25};
  struct Box {
    const char* name;
    bool on;
    double l[3];
  };
  const Box boxes[] = {{"free", false, {0, 0, 0}}, {"cube", true, {20, 20, 20}}, {"zero-edge", true, {20, 0, 20}},
                       {"negative-edge", true, {20, 20, -1}}, {"nan-edge", true, {std::nan(""), 20, 20}}};
  for (int model = 1; model <= 3; ++model)
    for (const Box& b : boxes) {
      mythos::SiteGeo g;
      mythos::g_error = "-";
      const bool ok = mythos::site_geo_from(model, geometry, b.on ? b.l : nullptr, "selftest", &g);
      printf("GEO model %d %s -> %d model %d g %.3f %.3f %.3f box_on %d %.1f %.1f %.1f: %s\n", model, b.name, ok ? 1 : 0, g.model, g.g_hb,
             g.g_k1, g.g_k2, g.box_on, g.box[0], g.box[1], g.box[2], mythos::g_error.c_str());
      if (ok != (!b.on || (b.l[0] > 0 && b.l[1] > 0 && b.l[2] > 0)) || (ok && (g.box_on != (b.on ? 1 : 0) || g.g_k2 != (model >= 2 ? geometry[2] : 0.0)))) return 73;
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (std::string(argv[1]) == "--index-lists") return index_lists_case();
  if (std::string(argv[1]) == "--device-buf") return device_buf_case();
  if (std::string(argv[1]) == "--md-plan") return md_plan_case();
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto hdr = rd<int32_t>(f, 6);
  const int model = hdr[0], n = hdr[1], nb = hdr[2], np = hdr[3], has_box = hdr[4], n_steps = hdr[5];
  if (model == 10) return martini_case(f, n, nb, np, has_box, n_steps);
  const auto seq = rd<int32_t>(f, n);
  const auto end32 = rd<int32_t>(f, n);
  const auto bonded = rd<int32_t>(f, 2 * (size_t)nb);
  const auto box = rd<double>(f, 3);
  const auto flat = rd<double>(f, np);
  auto c = rd<double>(f, 3 * (size_t)n);
  auto q = rd<double>(f, 4 * (size_t)n);
  const auto rna32 = model == 4 ? rd<int32_t>(f, n) : std::vector<int32_t>();
  fclose(f);
  std::vector<uint8_t> is_end(end32.begin(), end32.end());
  void* h = mythos_cpu_create(model, n, seq.data(), is_end.data(), nb, bonded.data(), has_box ? box.data() : nullptr, flat.data(), np);
  if (!h) return 3;
  if (model == 4) {
    std::vector<uint8_t> is_rna(rna32.begin(), rna32.end());
    mythos_cpu_set_types(h, is_rna.data());
  }
  mythos_cpu_build_pairs(h, c.data(), 3.25);
  double e[8];
  std::vector<double> dc(3 * (size_t)n), dq(4 * (size_t)n), tb(3 * (size_t)n);
  mythos_cpu_energy(h, c.data(), q.data(), e, dc.data(), dq.data(), tb.data());
  printf("E");
  for (double v : e) printf(" %.12e", v);
  double fs[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) fs[k] += dc[3 * (size_t)i + k];
  printf("\nFSUM %.3e %.3e %.3e\n", fs[0], fs[1], fs[2]);
  std::vector<double> p(3 * (size_t)n, 0.0), L(3 * (size_t)n, 0.0);
  const double inertia[3] = {1, 1, 1};
  double el[10];
  const int builds = mythos_cpu_langevin_run(h, c.data(), q.data(), p.data(), L.data(), n_steps, 0.005, 0.0987166667, 0.0394866667,
                                             0.0131622222, 1.0, inertia, 42, 0, 3.25, 0.3, 5, el);
  printf("MD builds %d E", builds);
  for (double v : el) printf(" %.10e", v);
  printf("\nX %.12e %.12e %.12e\n", c[0], c[3 * (size_t)(n - 1) + 2], q[4 * (size_t)(n / 2)]);
  mythos_cpu_destroy(h);
  return 0;
}
