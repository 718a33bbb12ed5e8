// libomega.so host side: the spectrum entry points -- omega_rfft, omega_spectra, omega_combine, the band
// tables, omega_chroma, the drum features and the post-processing.

#include "host.hpp"

extern "C" {

int omega_rfft(omega_ctx* c, const float* x, int64_t n, int32_t m, int32_t window, float* mag, float* cplx, int mem) try {
  if (!c || !x || (!mag && !cplx)) return OMEGA_EINVAL;
  if (m < 1) return fail(c, OMEGA_EINVAL, "rfft: length %d", m);
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  float* win = nullptr;
  int e = get_window(c, m, window, &win);
  if (e) return e;
  HostCall h(c, mem);
  const float* dx = h.in(x, (size_t)n * m * sizeof(float));
  float* dm = h.out(mag, (size_t)n * (m / 2 + 1));
  float* dc = h.out(cplx, (size_t)n * (m / 2 + 1) * 2);
  if (h.err) return h.err;
  if (!is_pow2_in(m, 512, 16384)) {  // other lengths: the mixed-radix transform (anyfft.hip)
    AnyFftParams ap{};
    ap.x = dx;
    ap.frame_stride = m;
    ap.n = n;
    ap.N = m;
    ap.win = win;
    ap.mag = dm;
    ap.cplx = dc;
    if ((e = run_any(c, ap, 0, c->stream))) return e;
    return h.finish();
  }
  RfftParams p{};
  p.x = dx;
  p.n = n;
  p.win = win;
  p.mag = dm;
  p.cplx = dc;
  for (int l = 0; l < kMaxLog2; ++l) p.tw[l] = c->d_tw[l];
  HIPC(c, launch_rfft(m, p, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_spectra(omega_ctx* c, const float* x, int64_t n, int32_t m, int32_t window, omega_bands* bands,
                  float* bands_out, double* chroma_out, float* mag_out, int mem) try {
  if (!c || !x || (!bands_out && !chroma_out && !mag_out)) return OMEGA_EINVAL;
  if (m != 8192) return fail(c, OMEGA_EUNSUP, "spectra: frame length %d unsupported (8192)", m);
  if (bands_out && (!bands || bands->op != OMEGA_BANDS_MAX || bands->n_bins != m / 2 + 1 || bands->n_valid > 512))
    return fail(c, OMEGA_EINVAL, "spectra: needs a MAX band table over %d bins with at most 512 bands", m / 2 + 1);
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  float* win = nullptr;
  int e = get_window(c, m, window, &win);
  if (e) return e;
  const int nbins = m / 2 + 1;
  const double df = (double)c->cfg.sample_rate / m;
  if (c->ctab.n_bins != nbins || c->ctab.df != df) {
    // chromagram.py:122-146 with offset 0: bins 20 < f < 8000, base class floor((69 + 12 log2(f/440)) mod 12)
    int lo = 0, nb = 0;
    mask_range(nbins, [&](int k) { return k * df; }, [](double f) { return f > 20 && f < 8000; }, &lo, &nb);
    const int hi = lo + nb;
    if (nb > 1408) return fail(c, OMEGA_EUNSUP, "spectra: %d chroma bins (at most 1408)", nb);
    std::vector<float4> w4(std::max(nb, 1));
    std::vector<float> w1(std::max(nb, 1));
    std::vector<int> base(std::max(nb, 1));
    std::vector<float> ra(std::max(nb, 1)), rg(std::max(nb, 1));  // SpectraParams::crec's a, g
    for (int k = lo; k < hi; ++k) {
      const double f = k * df;
      double cb = std::fmod(69 + 12 * std::log2(f / 440.0), 12.0);
      if (cb < 0) cb += 12.0;
      const int b = (int)cb;
      const double sw = f < 100 ? 0.5 : (f < 1000 ? 1.0 : (f < 4000 ? 0.8 : 0.6));
      float w[5];
      for (int o = -2; o <= 2; ++o) {
        const double d = std::fabs(cb - (b + o));
        w[o + 2] = (float)(std::exp(-0.5 * (d / 0.5) * (d / 0.5)) * sw);
      }
      w4[k - lo] = make_float4(w[0], w[1], w[2], w[3]);
      w1[k - lo] = w[4];
      base[k - lo] = b;
      const double u = cb - b;
      ra[k - lo] = (float)(std::exp(-2.0 * u * u) * sw);
      rg[k - lo] = (float)std::exp(4.0 * u);
    }
    std::vector<unsigned short> perm;
    std::vector<int> goff(13, 0);
    for (int b = 0; b < 12; ++b) {
      goff[b] = (int)perm.size();
      for (int i = 0; i < nb; ++i)
        if (base[i] == b) perm.push_back((unsigned short)i);
    }
    goff[12] = (int)perm.size();
    if (perm.empty()) perm.push_back(0);
    std::vector<float> rec(3 * perm.size());
    for (size_t j = 0; j < perm.size(); ++j) {
      const int i = perm[j];
      const int bin = lo + i;
      rec[3 * j] = ra[i];
      rec[3 * j + 1] = rg[i];
      std::memcpy(&rec[3 * j + 2], &bin, sizeof bin);  // the bin index's bits
    }
    for (void* q : {(void*)c->ctab.w4, (void*)c->ctab.w1, (void*)c->ctab.perm, (void*)c->ctab.goff,
                    (void*)c->ctab.rec})
      if (q) (void)hipFree(q);
    c->ctab = omega_ctx::ChromaTab{};
    HIPC(c, hipMalloc(&c->ctab.rec, rec.size() * sizeof(float)));
    HIPC(c, hipMemcpy(c->ctab.rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPC(c, hipMalloc(&c->ctab.w4, w4.size() * sizeof(float4)));
    HIPC(c, hipMalloc(&c->ctab.w1, w1.size() * sizeof(float)));
    HIPC(c, hipMalloc(&c->ctab.perm, perm.size() * sizeof(unsigned short)));
    HIPC(c, hipMalloc(&c->ctab.goff, goff.size() * sizeof(int)));
    HIPC(c, hipMemcpy(c->ctab.w4, w4.data(), w4.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->ctab.w1, w1.data(), w1.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->ctab.perm, perm.data(), perm.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->ctab.goff, goff.data(), goff.size() * sizeof(int), hipMemcpyHostToDevice));
    c->ctab.n_bins = nbins;
    c->ctab.df = df;
    c->ctab.lo = lo;
    c->ctab.hi = hi;
  }
  if (!c->n_cu) {
    hipDeviceProp_t prop;
    HIPC(c, hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
  }
  HostCall h(c, mem);
  const float* dx = h.in(x, (size_t)n * m * sizeof(float));
  float* db = h.out(bands_out, bands_out ? (size_t)n * bands->n_out : 0);
  double* dcr = h.out(chroma_out, (size_t)n * 12);
  float* dm = h.out(mag_out, (size_t)n * nbins);
  if (h.err) return h.err;
  SpectraParams p{};
  p.x = dx;
  p.n = n;
  p.stride = m;
  p.win = win;
  p.mag_out = dm;
  if (bands_out) {
    p.n_out = bands->n_out;
    p.n_valid = bands->n_valid;
    p.starts = bands->d_starts;
    p.ends = bands->d_ends;
    p.scale = bands->d_scale;
    p.bands_out = db;
  }
  p.c_lo = c->ctab.lo;
  p.c_hi = c->ctab.hi;
  p.cw4 = c->ctab.w4;
  p.cw1 = c->ctab.w1;
  p.cperm = c->ctab.perm;
  p.cgoff = c->ctab.goff;
  p.crec = c->ctab.rec;
  p.chroma_out = dcr;
  for (int l = 0; l < kMaxLog2; ++l) p.tw[l] = c->d_tw[l];
  const int grid = (int)std::min<int64_t>(n, 2 * (int64_t)c->n_cu);
  if (m == 8192)
    HIPC(c, launch_spectra_rf(m, p, c->stream));
  else
    HIPC(c, launch_spectra(m, p, grid, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_combine(omega_ctx* c, const float* const* mags, int64_t n_cf, float* out, int mem) try {
  if (!c || !mags || !out) return OMEGA_EINVAL;
  if (n_cf <= 0) return n_cf == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  const int T = c->cfg.target_bins;
  CombineParams p{};
  HostCall h(c, mem);  // (slots of its own, 20 .. 24: beside the slots of the calls that made the magnitudes)
  for (int r = 0; r < c->cfg.n_res; ++r) {
    p.nbins[r] = c->cfg.res[r].fft_size / 2 + 1;
    p.cw[r] = (float)c->cfg.res[r].weight;
    p.mag[r] = h.in(mags[r], (size_t)n_cf * p.nbins[r] * sizeof(float), 20 + r);
  }
  float* dout = h.out(out, (size_t)n_cf * T, 24);
  if (h.err) return h.err;
  p.n_cf = n_cf;
  p.T = T;
  p.own_off = c->d_own_off;
  p.own_rj = c->d_own_rj;
  p.own_frac = c->d_own_frac;
  p.out = dout;
  HIPC(c, launch_combine(p, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_bands_create(omega_ctx* c, int op, const int32_t* starts, const int32_t* ends, int32_t n_bands,
                       int32_t n_out, const double* scale, const double* bin_scale, int32_t n_bins, omega_bands** out) try {
  if (!c || !starts || !ends || !out || n_bands < 0 || n_out < 0 || n_bins <= 0) return OMEGA_EINVAL;
  if (op != OMEGA_BANDS_MAX && op != OMEGA_BANDS_MEAN) return fail(c, OMEGA_EINVAL, "unknown band op %d", op);
  HIPC(c, hipSetDevice(c->device));
  omega_bands* b = new (std::nothrow) omega_bands();
  if (!b) return OMEGA_ENOMEM;
  b->ctx = c;
  b->op = op;
  b->n_bands = n_bands;
  b->n_out = n_out;
  b->n_bins = n_bins;
  // MAX (pipeline.py:207-220): bands min(num_bands, len(table)); each one that fits the spectrum.
  // MEAN (freq_mapper.py:184-194): stops at the first band running past the spectrum.
  int nv = std::min(n_bands, n_out);
  if (op == OMEGA_BANDS_MEAN) {
    for (int i = 0; i < nv; ++i)
      if (ends[i] > n_bins) {
        nv = i;
        break;
      }
  }
  b->n_valid = nv;
  std::vector<int32_t> s(starts, starts + n_bands), en(ends, ends + n_bands);
  if (s.empty()) {
    s.push_back(0);
    en.push_back(1);
  }
  int e = upload(c, &b->d_starts, s);
  if (!e) e = upload(c, &b->d_ends, en);
  b->d_scale = nullptr;
  b->d_bin_scale = nullptr;
  if (!e && scale) {
    std::vector<float> sc(std::max(n_out, 1), 1.0f);
    for (int i = 0; i < std::min(n_bands, n_out); ++i) sc[i] = (float)scale[i];
    e = upload(c, &b->d_scale, sc);
  }
  if (!e && bin_scale) {
    std::vector<float> bs(bin_scale, bin_scale + n_bins);
    e = upload(c, &b->d_bin_scale, bs);
  }
  if (e) {
    delete b;
    return e;
  }
  *out = b;
  return 0;
} catch (...) {
  return guard_fail(c);
}

void omega_bands_destroy(omega_bands* b) { delete b; }  // device tables are owned by the context

int omega_bands_apply(omega_ctx* c, omega_bands* b, const float* spec, int64_t n, int64_t spec_stride, float* out,
                      int mem) try {
  if (!c || !b || !spec || !out) return OMEGA_EINVAL;
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);
  const Rows32 ds = h.rows32(spec, spec_stride, b->n_bins, n);
  float* dout = h.out(out, (size_t)n * b->n_out);
  if (h.err) return h.err;
  BandParams p{ds.base, n, spec_stride, b->n_bins, b->n_out, b->d_starts, b->d_ends, b->d_scale, b->d_bin_scale, b->op,
               b->n_valid, dout};
  HIPC(c, launch_bands(p, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"

namespace omega_host {
int get_chroma_mat(omega_ctx* c, int n_bins, double df, ChromaMat* out) {
  auto it = c->chroma_mats.find(n_bins);
  if (it == c->chroma_mats.end() || c->chroma_df != df) {
    // chromagram.py:122-146 with transposition offset 0: bins 20 < f < 8000
    int lo = 0, cnt = 0;
    mask_range(n_bins, [&](int k) { return k * df; }, [](double f) { return f > 20 && f < 8000; }, &lo, &cnt);
    const int hi = lo + cnt, nb = std::max(cnt, 1);
    std::vector<double> m(12 * (size_t)nb, 0.0);
    for (int k = lo; k < hi; ++k) {
      const double f = k * df;
      const double midi = 69 + 12 * std::log2(f / 440.0);
      double cb = std::fmod(midi, 12.0);
      if (cb < 0) cb += 12.0;
      const int base = (int)cb;
      const double sw = f < 100 ? 0.5 : (f < 1000 ? 1.0 : (f < 4000 ? 0.8 : 0.6));
      for (int o = -2; o <= 2; ++o) {
        const int tb = ((base + o) % 12 + 12) % 12;
        const double d = std::fabs(cb - (base + o));
        const double w = std::exp(-0.5 * (d / 0.5) * (d / 0.5));
        m[(size_t)tb * nb + (k - lo)] += w * sw;
      }
    }
    double* d = nullptr;
    HIPC(c, hipMalloc(&d, m.size() * sizeof(double)));
    HIPC(c, hipMemcpy(d, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice));
    if (it != c->chroma_mats.end()) (void)hipFree(it->second.first);
    c->chroma_mats[n_bins] = {d, {lo, hi}};
    c->chroma_df = df;
    it = c->chroma_mats.find(n_bins);
  }
  *out = {it->second.first, it->second.second.first, it->second.second.second};
  return 0;
}
}  // namespace omega_host

extern "C" {

int omega_chroma(omega_ctx* c, const float* spec, int64_t n, int32_t n_bins, double df, double* out_raw, int mem) try {
  if (!c || !spec || !out_raw || n_bins < 3 || !(df > 0)) return OMEGA_EINVAL;
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  ChromaMat m{};
  if (int e = get_chroma_mat(c, n_bins, df, &m)) return e;
  HostCall h(c, mem);
  const float* ds = h.in(spec, (size_t)n * n_bins * sizeof(float));
  double* dout = h.out(out_raw, (size_t)n * 12);
  if (h.err) return h.err;
  HIPC(c, launch_chroma(ds, n, n_bins, m.lo, m.hi, m.mat, dout, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_drum_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  if (!c->drum.bins) return 0;
  HIPC(c, hipSetDevice(c->device));
  for (int b = 0; b < 2; ++b) {
    HIPC(c, hipMemsetAsync(c->drum.len[b], 0, kDrumBands * sizeof(int), c->stream));
    HIPC(c, hipMemsetAsync(c->drum.pos[b], 0, sizeof(long long), c->stream));
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_drum_features(omega_ctx* c, const float* mag, int64_t n_frames, int32_t n_bins, int64_t mag_stride,
                        double sensitivity, double* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!mag || n_frames < 0 || n_bins < 2 || mag_stride < n_bins)
    return fail(c, OMEGA_EINVAL, "drum features: bad magnitude layout (n_bins %d, stride %lld)", n_bins,
                (long long)mag_stride);
  if (c->drum.bins && c->drum.bins != n_bins)
    return fail(c, OMEGA_EINVAL, "drum features: the stream has %d bins per frame, got %d (omega_drum_reset "
                "does not change it; create another context)", c->drum.bins, n_bins);
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  if (!c->drum.bins) {
    for (int b = 0; b < 2; ++b) {
      int e = dalloc(c, &c->drum.prev[b], (size_t)n_bins);
      if (!e) e = dalloc(c, &c->drum.hist[b], (size_t)kDrumBands * kDrumHist);
      if (!e) e = dalloc(c, &c->drum.len[b], kDrumBands);
      if (!e) e = dalloc(c, &c->drum.pos[b], 1);
      if (e) return e;
    }
    c->drum.bins = n_bins;
    const int e = omega_drum_reset(c);
    if (e) return e;
  }
  if (int e = grow(c, &c->drum.flux, &c->drum.flux_cap, n_frames * kDrumBands)) return e;
  HostCall h(c, mem);
  const Rows32 dm = h.rows32(mag, mag_stride, n_bins, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kDrumCols);
  if (h.err) return h.err;
  // drum_detection.py: bins int(f * len / nyquist) (:86-96, :240-259, :218-219), numpy slices clamp
  const double fs = c->cfg.sample_rate, ny = fs / 2;
  const double bands[kDrumBands][2] = {{20, 60}, {60, 120}, {2000, 5000}, {150, 400}, {400, 1000}, {2000, 8000},
                                       {8000, 15000}};
  const double mult[kDrumBands] = {2.8, 2.8, 2.8, 2.5, 2.3, 2.0, 0.0};  // :78, :295, :300, :305
  DrumParams p{};
  p.mag = dm.base;
  p.n = n_frames;
  p.stride = mag_stride;
  p.n_bins = n_bins;
  auto bin = [&](double f) { return std::min(n_bins, (int)(f * n_bins / ny)); };
  for (int b = 0; b < kDrumBands; ++b) {
    p.bs[b] = bin(bands[b][0]);
    p.be[b] = std::max(p.bs[b], bin(bands[b][1]));
    p.mult[b] = (float)(sensitivity * mult[b]);
  }
  p.cs = bin(150.0);
  p.ce = std::max(p.cs, bin(15000.0));
  p.fstep = 1.0 / ((2.0 * n_bins - 1.0) * (1.0 / fs));  // np.fft.rfftfreq(2 n - 1, 1 / fs) spacing
  const int a = c->drum.cur, b = a ^ 1;
  p.prev_in = c->drum.prev[a];
  p.prev_out = c->drum.prev[b];
  p.hist_in = c->drum.hist[a];
  p.hist_out = c->drum.hist[b];
  p.len_in = c->drum.len[a];
  p.len_out = c->drum.len[b];
  p.pos_in = c->drum.pos[a];
  p.pos_out = c->drum.pos[b];
  p.flux = c->drum.flux;
  p.out = dout;
  HIPC(c, launch_drum(p, c->stream));
  c->drum.cur = b;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_post_configure(omega_ctx* c, int32_t n_bins, const double* curve, const uint8_t* bass,
                         const float* comp_instr, const float* comp_vocal, const float* vocal_sup,
                         const int32_t* ranges, int32_t p_lo, int32_t p_hi, float p_gamma,
                         const int32_t* band_start, const int32_t* band_end, const double* band_smooth,
                         int32_t n_bands) try {
  if (!c) return OMEGA_EINVAL;
  if (n_bins < 1 || n_bins > kPostMaxBins || n_bands < 0 || n_bands > kPostMaxBands || !curve || !bass ||
      !comp_instr || !comp_vocal || !vocal_sup || !ranges || (n_bands && (!band_start || !band_end || !band_smooth)))
    return fail(c, OMEGA_EINVAL, "post configure: bad tables (n_bins %d, n_bands %d)", n_bins, n_bands);
  if (p_lo < 0 || p_hi < p_lo || p_hi > p_lo + 1 || p_hi >= n_bins)
    return fail(c, OMEGA_EINVAL, "post configure: percentile ranks %d, %d outside %d bins", p_lo, p_hi, n_bins);
  for (int b = 0; b < n_bands; ++b)
    if (band_start[b] < 0 || band_start[b] >= n_bins || band_end[b] > n_bins || band_end[b] < band_start[b])
      return fail(c, OMEGA_EINVAL, "post configure: band %d [%d, %d) outside %d bins", b, band_start[b],
                  band_end[b], n_bins);
  std::vector<EmaCoef> coef((size_t)n_bands);
  for (int b = 0; b < n_bands; ++b) {
    const double f = band_smooth[b];
    if (!(f >= 0.0 && f <= 1.0)) return fail(c, OMEGA_EINVAL, "post configure: band %d smoothing factor %g outside [0, 1]", b, f);
    coef[b] = EmaCoef{f, 1.0 - f, (float)f, (float)(1.0 - f)};
  }
  HIPC(c, hipSetDevice(c->device));
  PostParams p{};
  p.T = n_bins;
  p.nb = n_bands;
  p.be = ranges[0];
  p.vs = ranges[1];
  p.ve = ranges[2];
  p.hs = ranges[3];
  p.p_lo = p_lo;
  p.p_hi = p_hi;
  p.p_g = p_gamma;
  auto up = [&](auto** d, const auto* h, size_t n) {
    int e = dalloc(c, d, n);
    if (!e && n) {
      const hipError_t he = hipMemcpy(*d, h, n * sizeof(**d), hipMemcpyHostToDevice);
      if (he != hipSuccess) e = fail(c, OMEGA_EHIP, "post configure: %s", hipGetErrorString(he));
    }
    return e;
  };
  double* dc = nullptr;
  unsigned char* db = nullptr;
  float *d0 = nullptr, *d1 = nullptr, *dv = nullptr;
  EmaCoef* dsf = nullptr;
  int *dbs = nullptr, *dbe = nullptr;
  int e = up(&dc, curve, (size_t)n_bins);
  if (!e) e = up(&db, bass, (size_t)n_bins);
  if (!e) e = up(&d0, comp_instr, (size_t)n_bins);
  if (!e) e = up(&d1, comp_vocal, (size_t)n_bins);
  if (!e) e = up(&dv, vocal_sup, (size_t)n_bins);
  if (!e) e = up(&dbs, band_start, (size_t)n_bands);
  if (!e) e = up(&dbe, band_end, (size_t)n_bands);
  if (!e) e = up(&dsf, coef.data(), (size_t)n_bands);
  // the content ranges' leaf tables: [w][0] the count (at most 17 for 2048 bins), [w][1 ..] the leaves
  std::vector<unsigned> leaf_tab(4 * 32, 0u);
  const int rn[4] = {p.be, p.ve - p.vs, n_bins - p.hs, n_bins};
  for (int w = 0; w < 4; ++w) {
    std::vector<unsigned> lv;
    np_leaves(0, std::min(std::max(rn[w], 0), n_bins), 6, lv);  // (a range past the bins is not read)
    leaf_tab[32 * w] = (unsigned)lv.size();
    for (size_t i = 0; i < lv.size() && i < 31; ++i) leaf_tab[32 * w + 1 + i] = lv[i];
  }
  unsigned* dlt = nullptr;
  if (!e) e = up(&dlt, leaf_tab.data(), leaf_tab.size());
  if (!e) e = dalloc(c, &p.prev, (size_t)std::max(n_bands, 1) * 2);  // two EMA state buffers
  if (!e) e = dalloc(c, &p.has_prev, 4);
  if (e) return e;
  p.prev_out = p.prev + std::max(n_bands, 1);
  p.has_prev_out = p.has_prev + 2;
  p.curve = dc;
  p.bass = db;
  p.comp[0] = d0;
  p.comp[1] = d1;
  p.vsup = dv;
  p.bs = dbs;
  p.bend = dbe;
  p.sf = dsf;
  p.leaf_tab = dlt;
  c->post.p = p;
  return omega_post_reset(c);
} catch (...) {
  return guard_fail(c);
}

int omega_post_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  if (!c->post.p.T) return 0;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemsetAsync(std::min(c->post.p.has_prev, c->post.p.has_prev_out), 0, 4 * sizeof(int), c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_post_process(omega_ctx* c, const float* spectra, int64_t n_frames, int64_t stride, int32_t flags,
                       float bass_boost, float* spectrum_out, double* bands_out, int32_t* content_out) try {
  if (!c) return OMEGA_EINVAL;
  if (!c->post.p.T) return fail(c, OMEGA_EINVAL, "post process: omega_post_configure first");
  if (n_frames < 0 || stride < c->post.p.T || !spectra || !spectrum_out || (c->post.p.nb && !bands_out) ||
      n_frames > 0x7FFFFFFF)
    return fail(c, OMEGA_EINVAL, "post process: bad layout (n %lld, stride %lld, %d bins)", (long long)n_frames,
                (long long)stride, c->post.p.T);
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  PostParams p = c->post.p;
  p.in = spectra;
  p.n = n_frames;
  p.stride = stride;
  p.flags = flags;
  p.bass_boost = bass_boost;
  p.spec_out = spectrum_out;
  p.band_out = bands_out;
  p.content_out = content_out;
  // scratch: the raw band rows (+ the EMA's spare rows: post.hip post_ema_kernel), the per-frame dtype
  // flags, then (8-byte aligned) the EMA chunks' warm-up values at their boundaries and end values
  const int64_t rows = n_frames + kEmaSpareRows, nch = (n_frames + 63) / 64;
  const int64_t pre_off = (rows * (c->post.p.nb + 1) + 1) / 2 * 2;
  if (c->post.p.nb) {
    if (int e = grow(c, &c->post.raw, &c->post.raw_cap, pre_off + 4 * nch * c->post.p.nb + 4)) return e;
  }
  p.band_raw = c->post.raw;
  p.frame64 = reinterpret_cast<int*>(c->post.raw + rows * c->post.p.nb);
  p.ema_pre = reinterpret_cast<double*>(c->post.raw + pre_off);
  p.ema_end = p.ema_pre + nch * c->post.p.nb;
  HIPC(c, launch_post(p, c->stream));
  if (c->post.p.nb) {  // the EMA wrote the other state buffer: it is the next call's input
    std::swap(c->post.p.prev, c->post.p.prev_out);
    std::swap(c->post.p.has_prev, c->post.p.has_prev_out);
  }
  return 0;
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
