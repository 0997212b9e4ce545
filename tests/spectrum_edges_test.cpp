// ParseSpectrumEdges of include/jaybenne_amd.hpp from a command line, for tests/test_spectrum_host.py: prints the
// edges of argv[1] with %.17g, one per line, or "error: " and the exception's words.  Stand-alone: calls nothing of
// the library.
#include <cstdio>
#include <exception>

#include "../include/jaybenne_amd.hpp"

int main(int argc, char **argv) {
  try {
    for (double e : jaybenne_amd::ParseSpectrumEdges(argc > 1 ? argv[1] : "")) std::printf("%.17g\n", e);
  } catch (const std::exception &e) {
    std::printf("error: %s\n", e.what());
  }
  return 0;
}
