// The tonal entry points' argument checks and omega_tonal_state_size on the CPU
// (tests/test_tonal.py::test_abi_checks_its_arguments_without_a_device). The library named as the first argument is
// opened at run time; every answer below is decided before the library touches a device, so the program needs none
// (on a box without a GPU omega_create reports OMEGA_EHIP but still hands out the context). May be built with
// -fsanitize=address,undefined and run as it is.
#include <dlfcn.h>

#include <cstdio>

#include "../../include/omega.h"

static int check(const char* what, long long got, long long want) {
  std::printf("%s: %lld (want %lld)\n", what, got, want);
  return got == want ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) {
    std::printf("dlopen: %s\n", dlerror());
    return 2;
  }
  auto config_default = (void (*)(omega_config*))dlsym(h, "omega_config_default");
  auto create = (int (*)(const omega_config*, int, omega_ctx**))dlsym(h, "omega_create");
  auto destroy = (void (*)(omega_ctx*))dlsym(h, "omega_destroy");
  auto tn_default = (void (*)(omega_tonal_config*))dlsym(h, "omega_tonal_config_default");
  auto tn_configure = (int (*)(omega_ctx*, const omega_tonal_config*))dlsym(h, "omega_tonal_configure");
  auto tn_state = (int64_t (*)(void))dlsym(h, "omega_tonal_state_size");
  auto tn_features = (int (*)(omega_ctx*, const double*, int64_t, const int32_t*, const int32_t*, const double*, double*,
                              double*, double*, double*, double*, double*, int))dlsym(h, "omega_tonal_features");
  auto tn_spectra = (int (*)(omega_ctx*, const float*, int64_t, int32_t, double, const int32_t*, const int32_t*,
                             const double*, double*, double*, double*, double*, double*, double*, int))dlsym(
      h, "omega_tonal_spectra");
  if (!config_default || !create || !destroy || !tn_default || !tn_configure || !tn_state || !tn_features || !tn_spectra) {
    std::printf("a symbol is missing\n");
    return 2;
  }
  int bad = 0;
  bad |= check("state_size", tn_state(), 13);
  omega_tonal_config tc{77};
  tn_default(&tc);
  bad |= check("default genre", tc.genre, OMEGA_TONAL_POP);

  omega_config cfg;
  config_default(&cfg);
  omega_ctx* c = nullptr;
  const int rcode = create(&cfg, 0, &c);
  std::printf("omega_create: %d\n", rcode);
  if (!c) return 2;
  double raw[24] = {};
  float spec[16] = {};
  double rows[2 * OMEGA_TONAL_COLS];
  for (double& v : rows) v = -1;
  double state[13] = {-1};
  int32_t roll[2] = {0, 0}, first[2] = {1, 0};
  const int M = OMEGA_MEM_HOST;
  bad |= check("features before configure", tn_features(c, raw, 2, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  bad |= check("spectra before configure", tn_spectra(c, spec, 2, 8, 10.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M),
               OMEGA_EINVAL);
  bad |= check("configure: no context", tn_configure(nullptr, &tc), OMEGA_EINVAL);
  bad |= check("configure: no config", tn_configure(c, nullptr), OMEGA_EINVAL);
  for (int g : {-1, 6, 100}) {
    omega_tonal_config r{g};
    bad |= check("configure: unknown genre", tn_configure(c, &r), OMEGA_EINVAL);
  }
  bad |= check("features still unconfigured", tn_features(c, raw, 2, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  for (int g = OMEGA_TONAL_POP; g <= OMEGA_TONAL_OTHER; ++g) {
    omega_tonal_config r{g};
    bad |= check("configure", tn_configure(c, &r), OMEGA_OK);
  }
  bad |= check("features: no context", tn_features(nullptr, raw, 2, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  bad |= check("features: negative frames", tn_features(c, raw, -1, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  bad |= check("features: no chroma", tn_features(c, nullptr, 2, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  bad |= check("features: no rows", tn_features(c, raw, 2, roll, first, nullptr, state, nullptr, 0, 0, 0, 0, M), OMEGA_EINVAL);
  for (int r : {-12, 12, 1000}) {
    int32_t out_of_range[2] = {0, r};
    bad |= check("features: roll outside -11..11", tn_features(c, raw, 2, out_of_range, first, nullptr, state, rows, 0, 0, 0, 0, M),
                 OMEGA_EINVAL);
    bad |= check("spectra: roll outside -11..11",
                 tn_spectra(c, spec, 2, 8, 10.0, out_of_range, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  }
  bad |= check("spectra: no context", tn_spectra(nullptr, spec, 2, 8, 10.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M),
               OMEGA_EINVAL);
  bad |= check("spectra: negative frames", tn_spectra(c, spec, -1, 8, 10.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M),
               OMEGA_EINVAL);
  bad |= check("spectra: no spectra", tn_spectra(c, nullptr, 2, 8, 10.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M),
               OMEGA_EINVAL);
  bad |= check("spectra: no rows", tn_spectra(c, spec, 2, 8, 10.0, roll, first, nullptr, state, nullptr, 0, 0, 0, 0, M),
               OMEGA_EINVAL);
  bad |= check("spectra: 2 bins", tn_spectra(c, spec, 2, 2, 10.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  bad |= check("spectra: df 0", tn_spectra(c, spec, 2, 8, 0.0, roll, first, nullptr, state, rows, 0, 0, 0, 0, M), OMEGA_EINVAL);
  // the refused calls wrote nothing
  bad |= check("rows untouched", rows[0] == -1 && rows[2 * OMEGA_TONAL_COLS - 1] == -1, 1);
  bad |= check("state untouched", state[0] == -1, 1);
  destroy(c);
  std::printf(bad ? "FAIL\n" : "ok\n");
  return bad;
}
