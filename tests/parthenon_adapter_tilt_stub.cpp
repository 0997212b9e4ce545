// The stand-in for jb_set_source_tilt / jb_get_source_tilt that the Parthenon adapter's host-logic program links
// against beside the recording stand-in of tests/parthenon_adapter_test.cpp (adapters/parthenon/Makefile): the
// adapter's Initialize hands the deck key <jaybenne_amd> source_tilt to the library.  It keeps the mode it was given.
#include "jaybenne_amd.h"

static int g_source_tilt = JB_TILT_NONE;

extern "C" {
jb_status jb_set_source_tilt(jb_context *, int mode) {
  if (mode != JB_TILT_NONE && mode != JB_TILT_LINEAR) return JB_ERR_INVALID;
  g_source_tilt = mode;
  return JB_COMPLETE;
}
int jb_get_source_tilt(const jb_context *) { return g_source_tilt; }
}
