// omega_rhythm_configure's argument checks and omega_rhythm_state_size on the CPU
// (tests/test_rhythm.py::test_configure_checks_its_arguments_without_a_device). The library named as the first
// argument is opened at run time; every refusal below is decided before the library touches a device, so the program
// needs none (on a box without a GPU omega_create reports OMEGA_EHIP but still hands out the context).
#include <dlfcn.h>

#include <cstdio>
#include <vector>

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
  auto rh_default = (void (*)(omega_rhythm_config*))dlsym(h, "omega_rhythm_config_default");
  auto rh_configure =
      (int (*)(omega_ctx*, const omega_rhythm_config*, const double*, const int32_t*))dlsym(h, "omega_rhythm_configure");
  auto rh_state = (int64_t (*)(int32_t))dlsym(h, "omega_rhythm_state_size");
  auto rh_features = (int (*)(omega_ctx*, const float*, int64_t, const void*, int32_t, int64_t, int64_t, const double*,
                              double*, double*, int))dlsym(h, "omega_rhythm_features");
  if (!config_default || !create || !destroy || !rh_default || !rh_configure || !rh_state || !rh_features) {
    std::printf("a symbol is missing\n");
    return 2;
  }
  int bad = 0;
  bad |= check("state_size(513)", rh_state(513), 515);
  bad |= check("state_size(2)", rh_state(2), 4);
  bad |= check("state_size(8193)", rh_state(OMEGA_RHYTHM_MAX_BINS), 8195);
  bad |= check("state_size(0)", rh_state(0), 0);
  bad |= check("state_size(-7)", rh_state(-7), 0);
  omega_rhythm_config rc;
  rh_default(&rc);
  bad |= check("default n_bins", rc.n_bins, 513);
  bad |= check("default frame_len", rc.frame_len, 2048);

  omega_config cfg;
  config_default(&cfg);
  omega_ctx* c = nullptr;
  const int rcode = create(&cfg, 0, &c);
  std::printf("omega_create: %d\n", rcode);
  if (!c) return 2;
  std::vector<double> freqs(OMEGA_RHYTHM_MAX_BINS + 1);
  for (size_t i = 0; i < freqs.size(); ++i) freqs[i] = 46.875 * (double)i;
  int32_t edges[OMEGA_RHYTHM_EDGES] = {1, 2, 2, 3, 6, 11, 43, 86, 171, 427};
  bad |= check("no context", rh_configure(nullptr, &rc, freqs.data(), edges), OMEGA_EINVAL);
  bad |= check("no config", rh_configure(c, nullptr, freqs.data(), edges), OMEGA_EINVAL);
  bad |= check("no freqs", rh_configure(c, &rc, nullptr, edges), OMEGA_EINVAL);
  bad |= check("no edges", rh_configure(c, &rc, freqs.data(), nullptr), OMEGA_EINVAL);
  const int shapes[][2] = {{1, 2048}, {0, 2048}, {-3, 2048}, {OMEGA_RHYTHM_MAX_BINS + 1, 2048}, {513, 0}, {513, -1},
                           {513, OMEGA_RHYTHM_MAX_FRAME + 1}};
  for (const auto& s : shapes) {
    omega_rhythm_config r{s[0], s[1]};
    bad |= check("unbuilt shape", rh_configure(c, &r, freqs.data(), edges), OMEGA_EUNSUP);
  }
  int32_t e2[OMEGA_RHYTHM_EDGES];
  for (int i = 0; i < OMEGA_RHYTHM_EDGES; ++i) {
    for (int j = 0; j < OMEGA_RHYTHM_EDGES; ++j) e2[j] = edges[j];
    e2[i] = -1;
    bad |= check("negative edge", rh_configure(c, &rc, freqs.data(), e2), OMEGA_EINVAL);
    e2[i] = rc.n_bins + 1;
    bad |= check("edge past n_bins", rh_configure(c, &rc, freqs.data(), e2), OMEGA_EINVAL);
  }
  // nothing was configured by the refused calls
  float s[513] = {};
  double out[OMEGA_RHYTHM_COLS];
  bad |= check("features before configure", rh_features(c, s, 513, nullptr, 0, 1, 0, nullptr, nullptr, out, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  destroy(c);
  std::printf(bad ? "FAIL\n" : "ok\n");
  return bad;
}
