// The failure paths of afe_consumer.h's scope-bound helpers, as a program of its own for AddressSanitizer + UBSan on
// the host (tests/test_sanitizers.py builds and runs it with every device hidden, so that every HIP call fails: the
// path on which launch_render's hand-written event bracket used to leak its first event).  Holds with a device too.
#include <cstdio>

#include "afe_consumer.h"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
  using namespace afe;
  for (int round = 0; round < 3; round++) {
    {
      StreamTimer untimed(nullptr, false);          // nothing made, nothing recorded, nothing waited for
      CHECK(untimed.ok() && !untimed.e0 && !untimed.e1);
      float ms = -1.0f;
      CHECK(untimed.finish(AFE_OK, &ms) == AFE_OK && untimed.finish(AFE_ERR_HIP, &ms) == AFE_ERR_HIP && ms == -1.0f);
    }
    {
      StreamTimer timed(nullptr, true);
      float ms = -1.0f;
      if (!timed.ok()) {                            // an event could not be made: whatever was made goes with the scope
        CHECK(!timed.e1);
        CHECK(timed.finish(AFE_OK, &ms) == AFE_ERR_HIP && ms == -1.0f);
      } else {
        CHECK(timed.finish(AFE_ERR_HIP, &ms) == AFE_ERR_HIP && ms == -1.0f);     // a failed launch is not waited for
        CHECK(timed.finish(AFE_OK, &ms) == AFE_OK && ms >= 0.0f);
      }
    }
    {
      DevBuf a, b, c;
      const double src[4] = {1.0, 2.0, 3.0, 4.0};
      double back[4] = {0.0, 0.0, 0.0, 0.0};
      if (!a.alloc(0)) CHECK(!a.get() && a.capacity() == 0);   // (an empty request still allocates)
      if (b.upload(src, sizeof(src))) CHECK(b.download(back, sizeof(back)) && back[3] == 4.0);
      else CHECK(!b.download(back, sizeof(back)) && back[3] == 0.0);
      if (!c.alloc(~size_t(0) >> 1)) CHECK(!c.get() && c.capacity() == 0);   // refused with or without a device
      // a refusal is taken off the runtime and kept for its text: a request granted at a second attempt leaves nothing pending
      // (without a device the runtime answers every call, this one included, with its no-device error)
      int n_dev = 0;
      const bool have_device = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
      CHECK(c.get() || (last_refusal() != hipSuccess && (!have_device || hipGetLastError() == hipSuccess)));
    }
    int dev = -7;
    const int rc = pick_gfx950(round == 0 ? -1 : 1 << 20, &dev);
    CHECK(rc == AFE_OK ? dev >= 0 : (dev == -7 && (rc == AFE_ERR_NO_DEVICE || rc == AFE_ERR_HIP)));
    if (round > 0) CHECK(rc == AFE_ERR_NO_DEVICE);
  }
  (void)hipGetLastError();
  std::printf("ok\n");
  return 0;
}
