// buf_main.cpp -- afs_buf.h's owning buffer over a counting malloc / free allocator, as a CPU program
// (tests/test_buf_cpu.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer).
#define AFS_BUF_HOST_ONLY
#include "afs_buf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {

int g_live = 0, g_peak = 0, g_allocs = 0, g_frees = 0;
bool g_fail_next = false;

struct Counting {
  using error = int;
  static error alloc(void **p, size_t bytes) {
    if (g_fail_next) {
      g_fail_next = false;
      *p = reinterpret_cast<void *>(0x1);  // (a failing allocator may leave anything here)
      return 2;
    }
    *p = std::malloc(bytes);
    if (!*p) return 1;
    std::memset(*p, 0xA5, bytes);
    ++g_allocs;
    if (++g_live > g_peak) g_peak = g_live;
    return 0;
  }
  static void release(void *p) {
    std::free(p);
    ++g_frees;
    --g_live;
  }
};
using Buf = afs::Buf<Counting>;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("buf_main.cpp:%d: %s\n", __LINE__, #x);         \
      return 1;                                                   \
    }                                                             \
  } while (0)

int run() {
  {
    Buf b;
    CHECK(b.data() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(0) == 0 && b.data() == nullptr && g_allocs == 0);  // (nothing asked, nothing allocated)
    CHECK(b.reserve(100) == 0 && b.data() && b.capacity() == 100 && g_allocs == 1 && g_live == 1);
    void *p = b.data();
    b.as<char>()[99] = 7;  // (the whole block is writable)
    // below and at the capacity: no allocation, the block stays
    CHECK(b.reserve(40) == 0 && b.reserve(100) == 0 && b.data() == p && b.capacity() == 100 && g_allocs == 1);
    CHECK(b.as<char>()[99] == 7);
    // growth frees the old block before it allocates the new one: never two live blocks
    g_peak = g_live;
    CHECK(b.reserve(101) == 0 && b.capacity() == 101 && g_allocs == 2 && g_frees == 1 && g_live == 1 && g_peak == 1);
    b.as<char>()[100] = 1;
    CHECK(b.reserve(1 << 20) == 0 && b.capacity() == (size_t)1 << 20 && g_live == 1 && g_peak == 1);
    // a failing allocation: the old block is gone, the buffer empty; the next reserve recovers
    g_fail_next = true;
    CHECK(b.reserve((size_t)2 << 20) == 2 && b.data() == nullptr && b.capacity() == 0 && g_live == 0);
    CHECK(b.reserve(8) == 0 && b.data() && b.capacity() == 8 && g_live == 1);
    // two buffers: one live block each
    Buf c;
    CHECK(c.reserve(16) == 0 && g_live == 2);
    g_peak = g_live;
    CHECK(c.reserve(32) == 0 && b.reserve(64) == 0 && g_live == 2 && g_peak == 2);
    // move construction and assignment leave the source empty and free what the target held
    void *pc = c.data();
    Buf d(std::move(c));
    CHECK(c.data() == nullptr && c.capacity() == 0 && d.data() == pc && d.capacity() == 32 && g_live == 2);
    void *pb = b.data();
    d = std::move(b);
    CHECK(b.data() == nullptr && b.capacity() == 0 && d.data() == pb && d.capacity() == 64 && g_live == 1);
    CHECK(b.reserve(4) == 0 && g_live == 2);  // (a moved-from buffer is an empty one)
    d.release();
    CHECK(d.data() == nullptr && d.capacity() == 0 && g_live == 1);
  }
  // scope exit freed the rest
  CHECK(g_live == 0 && g_allocs == g_frees && g_allocs > 0);
  return 0;
}

}  // namespace

int main() {
  if (run()) return 1;
  std::printf("buf-ok\n");
  return 0;
}
