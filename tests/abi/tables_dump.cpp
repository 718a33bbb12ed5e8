// The host tables' pure builders on the CPU (tests/test_host_tables.py): reads one request per line from standard
// input (or from the file named as the first argument), evaluates csrc/design.cpp's builder and prints one line
// of float64 bit patterns (16 hex digits each).
//   tw period count  -> re[0] im[0] re[1] im[1] ...   twiddles64(period, count)
//   win kind M       -> w[0] ... w[M-1]               np_window64(kind, M), kind as OMEGA_WIN_*
//   sg w             -> W[0] ... W[w*w-1]             savgol_cubic(w), row p = the output's position in the window
//
// The library is built by hipcc, whose host compiler calls libm's cos and sin one by one, as the source says.
// g++ at -O1 and above merges cos(x) and sin(x) of one x into a sincos call, and glibc's sincos rounds the sine
// differently from its sin at a few arguments (one ulp; 2 pi 1955 / 4096 is one). So that this program evaluates
// the source's own operations under either compiler, g++ compiles design.cpp here without that pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("O0")
#endif
#include "../../audio-analyzer-omega_amd/csrc/design.cpp"

using namespace omega_host;

static void put(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  std::printf("%016llx ", (unsigned long long)u);
}

int main(int argc, char** argv) {
  std::FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  char what[8];
  int a = 0, b = 0;
  while (std::fscanf(in, "%7s", what) == 1) {
    if (!std::strcmp(what, "tw")) {
      if (std::fscanf(in, "%d %d", &a, &b) != 2 || a < 1 || b < 0 || b > (1 << 24)) return 3;
      for (const double2& t : twiddles64(a, b)) put(t.x), put(t.y);
    } else if (!std::strcmp(what, "win")) {
      if (std::fscanf(in, "%d %d", &a, &b) != 2 || b < 1 || b > (1 << 24)) return 3;
      for (double w : np_window64(a, b)) put(w);
    } else if (!std::strcmp(what, "sg")) {
      if (std::fscanf(in, "%d", &a) != 1 || a < 5 || a > 255 || !(a & 1)) return 3;
      std::vector<double> W((size_t)a * a);
      savgol_cubic(a, W.data());
      for (double w : W) put(w);
    } else {
      return 3;
    }
    std::printf("\n");
  }
  return 0;
}
