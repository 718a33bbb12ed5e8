// The meter panel entry points' argument checks on the CPU
// (tests/test_meter_panel.py::test_abi_checks_its_arguments_without_a_device). The library named as the first argument
// is opened at run time. The pure entry points, omega_meterpanel_configure's refusals and the update before any
// configure are decided before the library touches a device and run everywhere (without a GPU omega_create reports
// OMEGA_EHIP but still hands out the context). omega_meterpanel_update's own argument checks come behind a successful
// configure, which uploads the edges: they run only where omega_create returned OMEGA_OK, that is with the suite on a
// GPU machine. May be built with -fsanitize=address,undefined and run as it is.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>

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
  auto last_error = (const char* (*)(omega_ctx*))dlsym(h, "omega_last_error");
  auto mp_default = (void (*)(omega_meterpanel_config*))dlsym(h, "omega_meterpanel_config_default");
  auto mp_size = (int64_t (*)(const omega_meterpanel_config*))dlsym(h, "omega_meterpanel_state_size");
  auto mp_edges = (int (*)(const omega_meterpanel_config*, double*))dlsym(h, "omega_meterpanel_edges");
  auto mp_unpack = (int (*)(const omega_meterpanel_config*, const double*, double*, int32_t*, double*, int32_t*, double*,
                            int32_t*, double*, double*))dlsym(h, "omega_meterpanel_unpack");
  auto mp_configure = (int (*)(omega_ctx*, const omega_meterpanel_config*))dlsym(h, "omega_meterpanel_configure");
  auto mp_update = (int (*)(omega_ctx*, const void*, int64_t, int32_t, const double*, int64_t, int64_t, int32_t,
                            const double*, double*, int32_t*, double*, int))dlsym(h, "omega_meterpanel_update");
  if (!config_default || !create || !destroy || !last_error || !mp_default || !mp_size || !mp_edges || !mp_unpack ||
      !mp_configure || !mp_update) {
    std::printf("a symbol is missing\n");
    return 2;
  }
  int bad = 0;
  omega_meterpanel_config mc;
  std::memset(&mc, 0x55, sizeof mc);
  mp_default(&mc);
  mp_default(nullptr);
  bad |= check("default frame_len", mc.frame_len, 2048);
  bad |= check("default lengths", mc.level_len == 600 && mc.peak_len == 300 && mc.range_len == 300 && mc.n_bins == 60, 1);
  bad |= check("default range", mc.sample_rate == 48000.0 && mc.hist_lo == -60.0 && mc.hist_hi == 0.0, 1);
  bad |= check("state_size", mp_size(&mc), 16 + 600 + 300 + 300);
  bad |= check("state_size: no config", mp_size(nullptr), OMEGA_EINVAL);
  double edges[64];
  for (double& v : edges) v = -7;
  bad |= check("edges: no config", mp_edges(nullptr, edges), OMEGA_EINVAL);
  bad |= check("edges: no output", mp_edges(&mc, nullptr), OMEGA_EINVAL);
  bad |= check("edges untouched", edges[0] == -7 && edges[60] == -7, 1);
  bad |= check("edges", mp_edges(&mc, edges), OMEGA_OK);
  bad |= check("edges written", edges[0] == -60.0 && edges[37] == -23.0 && edges[60] == 0.0 && edges[61] == -7, 1);

  omega_config cfg;
  config_default(&cfg);
  omega_ctx* c = nullptr;
  const int rcode = create(&cfg, 0, &c);
  std::printf("omega_create: %d\n", rcode);
  if (!c) return 2;
  float frames[2 * 2048] = {};
  double meters[10] = {}, rows[2 * OMEGA_METERPANEL_COLS], state[16 + 1200];
  int32_t hist[2 * 60];
  for (double& v : rows) v = -1;
  for (double& v : state) v = -1;
  for (int32_t& v : hist) v = -1;
  const int M = OMEGA_MEM_HOST;
  bad |= check("update before configure", mp_update(c, frames, 2048, 0, meters, 2, 60, 0, nullptr, rows, hist, state, M),
               OMEGA_EINVAL);
  bad |= check("... with a message", std::strstr(last_error(c), "configure") != nullptr, 1);
  bad |= check("configure: no context", mp_configure(nullptr, &mc), OMEGA_EINVAL);
  bad |= check("configure: no config", mp_configure(c, nullptr), OMEGA_EINVAL);
  struct Case {
    const char* what;
    int want;
    void (*set)(omega_meterpanel_config&);
  };
  const Case cases[] = {
      {"configure: rate 0", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.sample_rate = 0; }},
      {"configure: negative rate", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.sample_rate = -48000; }},
      {"configure: negative frame_len", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.frame_len = -1; }},
      {"configure: frame_len 0", OMEGA_EUNSUP, [](omega_meterpanel_config& k) { k.frame_len = 0; }},
      {"configure: frame_len 16385", OMEGA_EUNSUP, [](omega_meterpanel_config& k) { k.frame_len = 16385; }},
      {"configure: level_len 0", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.level_len = 0; }},
      {"configure: level_len 4097", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.level_len = 4097; }},
      {"configure: peak_len -1", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.peak_len = -1; }},
      {"configure: range_len 4097", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.range_len = 4097; }},
      {"configure: n_bins 0", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.n_bins = 0; }},
      {"configure: n_bins 63", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.n_bins = 63; }},
      {"configure: hist_lo == hist_hi", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.hist_lo = 0; }},
      {"configure: hist_lo > hist_hi", OMEGA_EINVAL, [](omega_meterpanel_config& k) { k.hist_hi = -61; }},
  };
  for (const Case& k : cases) {
    omega_meterpanel_config r = mc;
    k.set(r);
    bad |= check(k.what, mp_configure(c, &r), k.want);
    bad |= check("... with a message", std::strstr(last_error(c), "meterpanel") != nullptr, 1);
    bad |= check("... state_size agrees", mp_size(&r), k.want);
  }
  bad |= check("update still unconfigured", mp_update(c, frames, 2048, 0, meters, 2, 60, 0, nullptr, rows, hist, state, M),
               OMEGA_EINVAL);
  if (rcode == OMEGA_OK) {  // (configure uploads the edges: it needs the device)
    bad |= check("configure", mp_configure(c, &mc), OMEGA_OK);
    bad |= check("update: negative frames", mp_update(c, frames, 2048, 0, meters, -1, 60, 0, nullptr, rows, hist, state, M),
                 OMEGA_EINVAL);
    bad |= check("update: too many frames",
                 mp_update(c, frames, 2048, 0, meters, (int64_t)1 << 31, 60, 0, nullptr, rows, hist, state, M), OMEGA_EINVAL);
    bad |= check("update: no frames", mp_update(c, nullptr, 2048, 0, meters, 2, 60, 0, nullptr, rows, hist, state, M),
                 OMEGA_EINVAL);
    bad |= check("update: no meters", mp_update(c, frames, 2048, 0, nullptr, 2, 60, 0, nullptr, rows, hist, state, M),
                 OMEGA_EINVAL);
    bad |= check("update: no rows", mp_update(c, frames, 2048, 0, meters, 2, 60, 0, nullptr, nullptr, hist, state, M),
                 OMEGA_EINVAL);
    bad |= check("update: stride 0", mp_update(c, frames, 0, 0, meters, 2, 60, 0, nullptr, rows, hist, state, M),
                 OMEGA_EINVAL);
    bad |= check("... with a message", std::strstr(last_error(c), "meterpanel") != nullptr, 1);
  }
  bad |= check("update: no context", mp_update(nullptr, frames, 2048, 0, meters, 2, 60, 0, nullptr, rows, hist, state, M),
               OMEGA_EINVAL);
  // the refused calls wrote nothing
  bad |= check("rows untouched", rows[0] == -1 && rows[2 * OMEGA_METERPANEL_COLS - 1] == -1, 1);
  bad |= check("hist untouched", hist[0] == -1 && hist[119] == -1, 1);
  bad |= check("state untouched", state[0] == -1 && state[1215] == -1, 1);
  destroy(c);
  std::printf(bad ? "FAIL\n" : "ok\n");
  return bad;
}
