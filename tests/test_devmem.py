"""The library's one owner of device and pinned memory (agri-fly_amd/csrc/afe_devmem.h) on the CPU: the header knows no
HIP, so here its policy is malloc with a ledger -- every request and every return is counted, and the k-th request can be
refused.  What the handles rely on: a refused growth leaves the buffer EMPTY (no pointer, no capacity), so the next call
asks again instead of launching on what an earlier failure left behind.  Built with AddressSanitizer + UBSan (leaks
included) and run directly.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include "afe_devmem.h"

static int g_live = 0, g_gets = 0, g_puts = 0, g_refuse_from = 0, g_refuse_to = 0;   // requests g_refuse_from .. g_refuse_to (1-based) are refused
static size_t g_last_bytes = 0;
struct Ledger {
  static void *get(size_t bytes) {
    g_gets++;
    g_last_bytes = bytes;
    if (g_gets >= g_refuse_from && g_gets <= g_refuse_to) return nullptr;
    void *p = std::malloc(bytes);
    std::memset(p, 0xab, bytes);          // the whole block is ours: the sanitizer would say otherwise
    g_live++;
    return p;
  }
  static void put(void *p) { g_puts++; g_live--; std::free(p); }
};
typedef afe::OwnedBuf<Ledger> Buf;

static void fresh(int refuse_from = 0, int refuse_to = 0) { g_gets = g_puts = 0; g_refuse_from = refuse_from; g_refuse_to = refuse_to; }
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  {   // alloc, then the end of the scope
    fresh();
    { Buf b; CHECK(b.alloc(100)); CHECK(b.get() && b.capacity() == 100 && g_live == 1); }
    CHECK(g_live == 0 && g_gets == 1 && g_puts == 1);
  }
  {   // alloc(0) asks for one byte; a second alloc gives the first block back before it asks
    fresh();
    Buf b;
    CHECK(b.alloc(0) && g_last_bytes == 1 && b.capacity() == 1 && b.get());
    CHECK(b.alloc(7) && g_gets == 2 && g_puts == 1 && g_live == 1 && b.capacity() == 7);
    CHECK(b.as<char>() == (char *)b.get());
  }
  CHECK(g_live == 0);
  {   // reserve: within the capacity nothing is asked and nothing reported; beyond it one return and one request of `want`
    fresh();
    Buf b;
    bool replaced = false;
    CHECK(b.reserve(100, 150, &replaced) && replaced && g_gets == 1 && g_puts == 0 && b.capacity() == 150);
    void *const before = b.get();
    replaced = false;
    CHECK(b.reserve(150, 400, &replaced) && !replaced && g_gets == 1 && g_puts == 0 && b.get() == before && b.capacity() == 150);
    CHECK(b.reserve(0, 0, &replaced) && !replaced && g_gets == 1);
    CHECK(b.reserve(151, 300, &replaced) && replaced && g_gets == 2 && g_puts == 1 && g_last_bytes == 300 && b.capacity() == 300 && g_live == 1);
  }
  CHECK(g_live == 0);
  {   // `want` refused, `need` granted
    fresh(2, 2);
    Buf b;
    CHECK(b.alloc(10));
    bool replaced = false;
    CHECK(b.reserve(200, 250, &replaced) && replaced && g_gets == 3 && g_puts == 1 && g_last_bytes == 200 && b.capacity() == 200 && b.get() && g_live == 1);
  }
  CHECK(g_live == 0);
  {   // both refused: empty, and the next, smaller request does ask (a handle's next call after a refused growth)
    fresh(2, 3);
    Buf b;
    CHECK(b.alloc(64));
    bool replaced = false;
    CHECK(!b.reserve(200, 250, &replaced) && replaced && g_gets == 3 && g_puts == 1 && b.get() == nullptr && b.capacity() == 0 && g_live == 0);
    CHECK(b.reserve(32, 40) && g_gets == 4 && g_last_bytes == 40 && b.capacity() == 40 && b.get() && g_live == 1);
    // need == want: one request only, and a refused alloc leaves the buffer empty as well
    fresh(1, 2);
    CHECK(!b.reserve(500, 500) && g_gets == 1 && g_puts == 1 && b.get() == nullptr && b.capacity() == 0);
    CHECK(!b.alloc(8) && g_gets == 2 && g_puts == 1 && b.get() == nullptr && b.capacity() == 0);
    b.reset();
    CHECK(g_puts == 1 && g_live == 0);
  }
  {   // moves: the source is empty afterwards, the target's old block goes back, every block goes back once
    fresh();
    {
      Buf a;
      CHECK(a.alloc(16));
      void *const pa = a.get();
      Buf b(std::move(a));
      CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == pa && b.capacity() == 16 && g_puts == 0);
      Buf c;
      CHECK(c.alloc(24));
      c = std::move(b);
      CHECK(b.get() == nullptr && b.capacity() == 0 && c.get() == pa && c.capacity() == 16 && g_puts == 1 && g_live == 1);
      Buf &self = c;
      c = std::move(self);
      CHECK(c.get() == pa && c.capacity() == 16 && g_puts == 1);
      CHECK(a.reserve(4, 4) && g_live == 2);       // a moved-from buffer is an empty one: usable
    }
    CHECK(g_live == 0 && g_gets == 3 && g_puts == 3);
  }
  std::printf("ok\n");
  return 0;
}
'''


def test_owned_buffer_rules_under_sanitizers(tmp_path):
    src = tmp_path / "devmem.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "devmem"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-self-move", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "agri-fly_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip() == "ok" and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])
