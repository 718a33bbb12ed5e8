// The frame-batch layer on the CPU (tests/test_frames.py): reads one case per line from standard input (or from
// the file named as the first argument), evaluates csrc/frames.hpp on it and prints one line of numbers.
//   r f64 n_frames width stride f0
//     a Rows batch (and, for f64 = 0, the Rows32 one) over a buffer whose element k holds the value k
//     -> span_bytes  byte offset of from(f0)  then, for the rows of from(f0), every at(f, i), row(f)[i] and
//        row_as<T>(f)[i] (and Rows32's row(f)[i]) -- one number where they agree, else the line ends in "mismatch"
//   c n_frames per out       out: 0 no state_out, 1 a buffer of its own, 2 state_in's buffer
//     -> per launch of chain_chunks: f0 count read write copy_back, the buffers by ChainBuf's numbers
#include <cstdio>
#include <vector>

#include "../../audio-analyzer-omega_amd/csrc/frames.hpp"

using namespace omega;

template <class T>
static bool rows_case(int n_frames, int width, int stride, int f0) {
  const Rows shape{nullptr, stride, sizeof(T) == 8};
  const size_t span = shape.span_bytes(n_frames, width);
  std::vector<T> buf(span / sizeof(T));  // (exactly the span: a read past it is the sanitizer's to report)
  for (size_t k = 0; k < buf.size(); ++k) buf[k] = (T)k;
  const Rows all{buf.data(), stride, sizeof(T) == 8};
  const Rows part = all.from(f0);
  const Rows32 all32{reinterpret_cast<const float*>(buf.data()), stride};
  const Rows32 part32 = all32.from(f0);
  bool same = sizeof(T) == 8 || (all32.span_bytes(n_frames, width) == span &&
                                 static_cast<const void*>(part32.base) == part.base);
  std::printf("%zu %td", span, static_cast<const char*>(part.base) - reinterpret_cast<const char*>(buf.data()));
  for (int f = 0; f < n_frames - f0; ++f) {
    const Row row = part.row(f);
    for (int i = 0; i < width; ++i) {
      const double v = part.at(f, i);
      same = same && row[i] == v && (double)part.row_as<T>(f)[i] == v;
      same = same && (sizeof(T) == 8 || (double)part32.row(f)[i] == v);
      std::printf(" %.17g", v);
    }
  }
  std::printf(same ? "\n" : " mismatch\n");
  return true;
}

static bool chain_case(long long n_frames, long long per, int out) {
  if (per < 1 || out < 0 || out > 2) return false;
  chain_chunks(n_frames, per, out != 0, out == 2, [](int64_t f0, int64_t count, ChainBuf read, ChainStep s) {
    std::printf("%lld %lld %d %d %d ", (long long)f0, (long long)count, (int)read, (int)s.write, (int)s.copy_back);
    return 0;
  });
  std::printf("\n");
  return true;
}

int main(int argc, char** argv) {
  std::FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  char type;
  while (std::fscanf(in, " %c", &type) == 1) {
    bool ok = false;
    if (type == 'r') {
      int f64, n, width, stride, f0;
      if (std::fscanf(in, "%d %d %d %d %d", &f64, &n, &width, &stride, &f0) != 5) return 2;
      if (n < 0 || width < 1 || stride < 1 || f0 < 0 || f0 > n) return 2;
      ok = f64 ? rows_case<double>(n, width, stride, f0) : rows_case<float>(n, width, stride, f0);
    } else if (type == 'c') {
      long long n, per;
      int out;
      if (std::fscanf(in, "%lld %lld %d", &n, &per, &out) != 3) return 2;
      ok = chain_case(n, per, out);
    }
    if (!ok) return 2;
  }
  return 0;
}
