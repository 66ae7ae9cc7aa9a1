// Host-side check of the entry points of mickey_amd/csrc/mk_train_bn.hip: every call below hands over bad arguments (null, misaligned,
// C = 6, M = 0, a row stride below C ...) and must come back with MK_ERR_INVALID_ARGUMENT before anything is launched, so the program
// needs no GPU.  Built with the host sanitizers, it also shows that the argument checks themselves read nothing they should not:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/check_train_bn_args.cpp mickey_amd/csrc/mk_train_bn.hip -o check_train_bn_args && ./check_train_bn_args
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/mickey_hip.h"

static char g_error[512];
void mk_set_error(const char* fmt, ...) {   // the library's own lives in another translation unit
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

static int failures = 0;
static void expect(int rc, int want, const char* fn, const char* what) {
  const bool named = want == MK_OK || strstr(g_error, fn) != nullptr;
  if (rc != want || !named) {
    printf("FAIL %s (%s): returned %d, expected %d, message '%s'\n", fn, what, rc, want, g_error);
    ++failures;
  }
  g_error[0] = 0;
}

int main() {
  alignas(16) static float buf[64];
  float* ok = buf;
  float* odd = buf + 1;                                  // 4-byte aligned only
  unsigned char* mask = (unsigned char*)buf;
  long long nbt = 0;
  struct F { const float* x; long long ldx; const float* gamma; const float* resid; long long ldr; float* rm; long long* nbt; float mom;
             float eps; float* work; float* y; long long ldy; unsigned char* mask; int M, C, relu, training; };
  const F good = {ok, 64, ok, ok, 64, ok, &nbt, 0.1f, 1e-5f, ok, ok, 64, mask, 100, 64, 1, 1};
  auto fwd = [&](F a, const char* what) {
    expect(mk_train_bn_fwd(a.x, a.ldx, a.gamma, ok, a.resid, a.ldr, a.rm, ok, a.nbt, a.mom, a.eps, a.work, a.y, a.ldy, ok, ok, a.mask, a.M,
                           a.C, a.relu, a.training, nullptr),
           MK_ERR_INVALID_ARGUMENT, "mk_train_bn_fwd", what);
  };
  F a = good; a.x = nullptr; fwd(a, "null x");
  a = good; a.gamma = nullptr; fwd(a, "null gamma");
  a = good; a.y = nullptr; fwd(a, "null y");
  a = good; a.rm = nullptr; fwd(a, "null running_mean");
  a = good; a.nbt = nullptr; fwd(a, "null batch counter in training");
  a = good; a.work = nullptr; fwd(a, "null work in training");
  a = good; a.x = odd; fwd(a, "misaligned x");
  a = good; a.y = odd; fwd(a, "misaligned y");
  a = good; a.resid = odd; fwd(a, "misaligned resid");
  a = good; a.mask = mask + 4; fwd(a, "misaligned mask");
  a = good; a.C = 6; fwd(a, "C = 6");
  a = good; a.C = 0; fwd(a, "C = 0");
  a = good; a.C = 1028; fwd(a, "C = 1028");
  a = good; a.M = 0; fwd(a, "M = 0");
  a = good; a.M = 0; a.training = 0; fwd(a, "M = 0, eval");
  a = good; a.M = 1; fwd(a, "M = 1 in training");
  a = good; a.ldx = 60; fwd(a, "ldx < C");
  a = good; a.ldy = 66; fwd(a, "ldy no multiple of 4");
  a = good; a.ldr = 32; fwd(a, "ldr < C");
  a = good; a.eps = -1.f; fwd(a, "negative eps");
  a = good; a.mom = -1.f; fwd(a, "negative momentum");
  a = good; a.relu = 0; fwd(a, "a mask without a ReLU");

  struct B { const float* g; long long ldg; const float* x; long long ldx; const float* mean; const unsigned char* mask; float* work; float* gx;
             long long ldgx; float* gresid; long long ldgr; float eps; int M, C, training; };
  const B goodb = {ok, 64, ok, 64, ok, mask, ok, ok, 64, ok, 64, 1e-5f, 100, 64, 1};
  auto bwd = [&](B b, const char* what, int want = MK_ERR_INVALID_ARGUMENT) {
    expect(mk_train_bn_bwd(b.g, b.ldg, b.x, b.ldx, ok, b.mean, ok, b.mask, b.work, b.gx, b.ldgx, b.gresid, b.ldgr, want == MK_OK ? nullptr : ok,
                           want == MK_OK ? nullptr : ok, b.eps, b.M, b.C, b.training, nullptr),
           want, "mk_train_bn_bwd", what);
  };
  B b = goodb; b.g = nullptr; bwd(b, "null g");
  b = goodb; b.x = nullptr; bwd(b, "null x");
  b = goodb; b.mean = nullptr; bwd(b, "null mean");
  b = goodb; b.work = nullptr; bwd(b, "null work");
  b = goodb; b.g = odd; bwd(b, "misaligned g");
  b = goodb; b.gx = odd; bwd(b, "misaligned gx");
  b = goodb; b.gresid = odd; bwd(b, "misaligned gresid");
  b = goodb; b.mask = mask + 8; bwd(b, "misaligned mask");
  b = goodb; b.C = 6; bwd(b, "C = 6");
  b = goodb; b.M = 0; bwd(b, "M = 0");
  b = goodb; b.M = 1; bwd(b, "M = 1 in training");
  b = goodb; b.ldg = 62; bwd(b, "ldg no multiple of 4");
  b = goodb; b.ldgx = 32; bwd(b, "ldgx < C");
  b = goodb; b.eps = -1.f; bwd(b, "negative eps");
  b = goodb; b.gx = nullptr; b.gresid = nullptr; bwd(b, "nothing wanted: nothing launched", MK_OK);

  if (mk_train_bn_chunk_rows() <= 0 || mk_train_bn_chunks(0) != 0 || mk_train_bn_chunks(1) != 1 ||
      mk_train_bn_chunks(mk_train_bn_chunk_rows() + 1) != 2 || mk_train_bn_work_floats(0, 64) != 0 || mk_train_bn_work_floats(100, 0) != 0) {
    printf("FAIL chunk queries\n");
    ++failures;
  }
  printf(failures ? "%d FAILED\n" : "check_train_bn_args: all argument checks hold\n", failures);
  return failures ? 1 : 0;
}
