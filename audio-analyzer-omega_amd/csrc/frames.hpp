// A batch of frames as the feature families see it, and the plan of a call's chained launches. Pure: no HIP
// calls, usable from host and device code, CPU-tested through tests/abi/frames_dump.cpp (tests/test_frames.py).
//
// Rows: row f of the batch starts at element f * stride of `base`; the elements are float32, or float64 when
// f64. Rows32 is its float32-only sibling for the spectra. Every family's params struct carries these in place
// of a pointer / stride / flag triple, and the offset of a row and the bytes a batch spans are computed here
// and nowhere else: the host stages span_bytes() (HostCall::rows) and hands each launch from(f0), the kernels
// read at() or row(). The stride may be smaller than the width (overlapping `unfold` rows); a null base (no
// audio) stays null through from().
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define OMEGA_HD __host__ __device__ __forceinline__
#else
#define OMEGA_HD inline
#endif

namespace omega {

// the elements from a batch's first to the last one a batch of n_frames rows of `width` touches
OMEGA_HD size_t span_elems(int64_t n_frames, int64_t stride, int64_t width) {
  return n_frames > 0 ? (size_t)((n_frames - 1) * stride + width) : 0;
}

// one row of a Rows batch: r[i] widens as at() does
struct Row {
  const void* p;
  int f64;
  OMEGA_HD double operator[](int64_t i) const {
    return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
  }
};

struct Rows {
  const void* base = nullptr;
  int64_t stride = 0;  // elements from one row to the next
  int f64 = 0;
  OMEGA_HD size_t el() const { return f64 ? 8 : 4; }
  template <class T>  // row f where the caller knows the element type
  OMEGA_HD const T* row_as(int64_t f) const {
    return static_cast<const T*>(base) + f * stride;
  }
  OMEGA_HD Row row(int64_t f) const { return {static_cast<const char*>(base) + (size_t)(f * stride) * el(), f64}; }
  OMEGA_HD double at(int64_t f, int64_t i) const {
    const int64_t k = f * stride + i;
    return f64 ? static_cast<const double*>(base)[k] : (double)static_cast<const float*>(base)[k];
  }
  OMEGA_HD Rows from(int64_t f0) const { return {base ? row(f0).p : nullptr, stride, f64}; }
  OMEGA_HD size_t span_bytes(int64_t n_frames, int64_t width) const {
    return span_elems(n_frames, stride, width) * el();
  }
};

struct Rows32 {
  const float* base = nullptr;
  int64_t stride = 0;
  OMEGA_HD const float* row(int64_t f) const { return base + f * stride; }
  OMEGA_HD Rows32 from(int64_t f0) const { return {base ? row(f0) : nullptr, stride}; }
  OMEGA_HD size_t span_bytes(int64_t n_frames, int64_t width) const {
    return span_elems(n_frames, stride, width) * sizeof(float);
  }
};

// ---- the state chain of a call that takes several launches ----
// Launch i reads the state launch i - 1 wrote (the first: the caller's state_in) and no launch may read and write
// one buffer, so the launches alternate between two blobs of the context, k = i & 1. Only the call's last launch
// touches the caller's state_out: directly, or -- where state_out is state_in's buffer, which the launch may
// still be reading -- through blob k and a copy behind the launch. No state_out: the last launch writes nowhere.
enum ChainBuf : int { kChainNone = -1, kChainBlob0 = 0, kChainBlob1 = 1, kChainIn = 2, kChainOut = 3 };
struct ChainStep {
  ChainBuf write;  // where the launch writes its state (kChainNone: nowhere)
  bool copy_back;  // the blob it wrote is copied to the caller's state_out behind the launch
};
inline ChainStep chain_step(bool last, bool has_out, bool out_is_in, int k) {
  const ChainBuf blob = k ? kChainBlob1 : kChainBlob0;
  if (!last) return {blob, false};
  if (!has_out) return {kChainNone, false};
  if (!out_is_in) return {kChainOut, false};
  return {blob, true};
}
// body(f0, count, read, step) over [0, n_frames) in launches of at most `per` frames, `read` the buffer the launch
// takes its state from; stops at the first error
template <class F>
int chain_chunks(int64_t n_frames, int64_t per, bool has_out, bool out_is_in, F body) {
  ChainBuf read = kChainIn;
  int k = 0;
  for (int64_t f0 = 0; f0 < n_frames; f0 += per, k ^= 1) {
    const int64_t count = per < n_frames - f0 ? per : n_frames - f0;
    const ChainStep s = chain_step(f0 + count == n_frames, has_out, out_is_in, k);
    if (int e = body(f0, count, read, s)) return e;
    read = s.write;
  }
  return 0;
}

}  // namespace omega
