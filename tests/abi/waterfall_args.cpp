// The waterfall entry points' argument checks, omega_waterfall_mapping and omega_waterfall_state_size on the CPU
// (tests/test_waterfall.py::test_abi_checks_its_arguments_without_a_device). The library named as the first argument
// is opened at run time; every answer below is decided before the library touches a device, so the program needs
// none (on a box without a GPU omega_create reports OMEGA_EHIP but still hands out the context). May be built with
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
  auto wf_default = (void (*)(omega_waterfall_config*))dlsym(h, "omega_waterfall_config_default");
  auto wf_mapping = (int (*)(double, int32_t, double, double, int32_t*, int32_t*))dlsym(h, "omega_waterfall_mapping");
  auto wf_configure = (int (*)(omega_ctx*, const omega_waterfall_config*))dlsym(h, "omega_waterfall_configure");
  auto wf_state = (int64_t (*)(void))dlsym(h, "omega_waterfall_state_size");
  auto wf_rows = (int (*)(omega_ctx*, const void*, int64_t, int32_t, int64_t, int32_t, double, int32_t, const double*,
                          double*, double*, void*, uint8_t*, int))dlsym(h, "omega_waterfall_rows");
  auto wf_colors = (int (*)(omega_ctx*, const void*, int64_t, int32_t, int64_t, int32_t, int32_t, uint8_t*, int))dlsym(
      h, "omega_waterfall_colors");
  if (!config_default || !create || !destroy || !wf_default || !wf_mapping || !wf_configure || !wf_state || !wf_rows ||
      !wf_colors) {
    std::printf("a symbol is missing\n");
    return 2;
  }
  int bad = 0;
  bad |= check("state_size", wf_state(), 3 + 2 * OMEGA_WATERFALL_HISTORY + 2);
  omega_waterfall_config wc;
  wf_default(&wc);
  bad |= check("default n_bins", wc.n_bins, 1025);
  bad |= check("default first_bin", wc.first_bin, 1);
  bad |= check("default n_cells", wc.n_cells, 853);

  // the mapping at the four rates of the golden file, and its refusals
  const struct {
    double fs;
    int n, lo, hi;
  } maps[] = {{48000, 2048, 1, 854}, {96000, 16384, 4, 3414}, {44100, 2048, 1, 929}, {32000, 2048, 2, 1024}};
  for (const auto& m : maps) {
    int32_t lo = -1, hi = -1;
    bad |= check("mapping", wf_mapping(m.fs, m.n, 20, 20000, &lo, &hi), OMEGA_OK);
    bad |= check("  first_bin", lo, m.lo);
    bad |= check("  end_bin", hi, m.hi);
  }
  int32_t lo = -1, hi = -1;
  bad |= check("mapping above Nyquist", wf_mapping(48000, 2048, 30000, 40000, &lo, &hi), OMEGA_OK);
  bad |= check("  first_bin", lo, 0);
  bad |= check("  end_bin", hi, 1024);
  bad |= check("mapping without outputs", wf_mapping(48000, 2048, 20, 20000, nullptr, nullptr), OMEGA_OK);
  bad |= check("mapping rate 0", wf_mapping(0, 2048, 20, 20000, &lo, &hi), OMEGA_EINVAL);
  bad |= check("mapping size 1", wf_mapping(48000, 1, 20, 20000, &lo, &hi), OMEGA_EINVAL);

  omega_config cfg;
  config_default(&cfg);
  omega_ctx* c = nullptr;
  const int rcode = create(&cfg, 0, &c);
  std::printf("omega_create: %d\n", rcode);
  if (!c) return 2;
  float s[8] = {};
  double stats[OMEGA_WATERFALL_COLS] = {-1, -1, -1, -1, -1, -1, -1};
  float rows[8] = {-1};
  uint8_t rgb[24] = {7};
  bad |= check("rows before configure", wf_rows(c, s, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("configure: no context", wf_configure(nullptr, &wc), OMEGA_EINVAL);
  bad |= check("configure: no config", wf_configure(c, nullptr), OMEGA_EINVAL);
  const int shapes[][3] = {{0, 0, 1},   {-5, 0, 1},   {OMEGA_WATERFALL_MAX_BINS + 1, 0, 1}, {1025, 1, 0}, {1025, 1, -3},
                           {1025, -1, 4}, {1025, 1, 1025}, {1025, 1025, 1},                   {8, 7, 2}};
  for (const auto& q : shapes) {
    omega_waterfall_config r{q[0], q[1], q[2]};
    bad |= check("unbuilt shape", wf_configure(c, &r), OMEGA_EUNSUP);
  }
  bad |= check("rows still unconfigured", wf_rows(c, s, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  omega_waterfall_config ok{8, 1, 6};
  bad |= check("configure 8 bins", wf_configure(c, &ok), OMEGA_OK);
  omega_waterfall_config full{OMEGA_WATERFALL_MAX_BINS, 0, OMEGA_WATERFALL_MAX_BINS};
  bad |= check("configure the largest shape", wf_configure(c, &full), OMEGA_OK);
  bad |= check("configure 8 bins again", wf_configure(c, &ok), OMEGA_OK);
  bad |= check("rows: no context", wf_rows(nullptr, s, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("rows: negative frames", wf_rows(c, s, 8, 0, -1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("rows: no spectra", wf_rows(c, nullptr, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("rows: stride 0", wf_rows(c, s, 0, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("rows: no stats", wf_rows(c, s, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, nullptr, rows, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("rows: no rows", wf_rows(c, s, 8, 0, 1, 1, 0.0, 0, nullptr, nullptr, stats, nullptr, rgb, OMEGA_MEM_HOST),
               OMEGA_EINVAL);
  bad |= check("colors: no context", wf_colors(nullptr, s, 8, 0, 1, 8, 0, rgb, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: negative rows", wf_colors(c, s, 8, 0, -1, 8, 0, rgb, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: negative cells", wf_colors(c, s, 8, 0, 1, -8, 0, rgb, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: no intensity", wf_colors(c, nullptr, 8, 0, 1, 8, 0, rgb, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: no output", wf_colors(c, s, 8, 0, 1, 8, 0, nullptr, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: stride 0", wf_colors(c, s, 0, 0, 1, 8, 0, rgb, OMEGA_MEM_HOST), OMEGA_EINVAL);
  bad |= check("colors: no rows", wf_colors(c, nullptr, 8, 0, 0, 8, 0, nullptr, OMEGA_MEM_HOST), OMEGA_OK);
  // the refused calls wrote nothing
  bad |= check("stats untouched", stats[0] == -1 && stats[6] == -1, 1);
  bad |= check("rows untouched", rows[0] == -1, 1);
  bad |= check("rgb untouched", rgb[0], 7);
  destroy(c);
  std::printf(bad ? "FAIL\n" : "ok\n");
  return bad;
}
