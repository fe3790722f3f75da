// Stand-alone check of csrc/workspace.h (Workspace, ParamLayout) against offsets computed here
// independently as a running sum rounded up.  Built by tests/test_workspace_host.py with
// -fsanitize=address,undefined; exit status 0 = every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "workspace.h"

using ppo::ParamLayout;
using ppo::Workspace;

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

static int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct Net {  // destinations inside arrays of a heap struct, as the contexts hold them
  float *h[3];
  uint16_t *w16[2][2];  // bf16-sized elements
  void *raw;
};
struct Ctx {
  Net net[2];
  char *bytes;
  float *tail_buf;
};

// The expected offsets: a running sum, each start rounded up to `align`.
struct Expect {
  int64_t align, at = 0;
  std::vector<int64_t> offs;
  void add(int64_t bytes, int64_t slack) {
    offs.push_back(at);
    at = round_up(at + bytes, align) + slack;
  }
};

static void check_arena(int64_t align, int64_t slack, int64_t tail) {
  std::unique_ptr<Ctx> ctx(new Ctx());
  Workspace ws(align, slack, tail);
  Expect ex{align};
  std::vector<void *> order;  // every destination, in take order
  auto note = [&](void *dst, int64_t bytes, int64_t s) {
    order.push_back(dst);
    ex.add(bytes, s);
  };
  auto held = [](void *dst) {  // the pointer a destination holds, whatever its type
    char *p;
    std::memcpy(&p, dst, sizeof p);
    return p;
  };
  for (int z = 0; z < 2; ++z) {
    Net &n = ctx->net[z];
    for (int l = 0; l < 3; ++l) {
      const int64_t b = 4 * (100 + 37 * l + z);  // odd extents: no multiple of the alignment
      ws.take(&n.h[l], b);
      note(&n.h[l], b, slack);
    }
    for (int d = 0; d < 2; ++d)
      for (int e = 0; e < 2; ++e) {
        const int64_t b = 2 * (257 + d + 2 * e);
        ws.take(&n.w16[d][e], b, 0);  // packed: the slack overridden to zero
        note(&n.w16[d][e], b, 0);
      }
    ws.take(&n.raw, 0);  // a zero-byte buffer still gets an aligned start of its own
    note(&n.raw, 0, slack);
  }
  ws.take(&ctx->bytes, 1, 3 * align);  // a slack override larger than the default
  note(&ctx->bytes, 1, 3 * align);
  ws.take(&ctx->tail_buf, 4 * 1000);
  note(&ctx->tail_buf, 4 * 1000, slack);

  CHECK(ws.bytes() == ex.at + tail);  // bytes() includes the tail
  CHECK(ws.bytes() >= ex.offs.back() + 4 * 1000 + tail);

  // two `align`-aligned bases inside one real allocation
  std::vector<char> arena(static_cast<size_t>(ws.bytes() + 9 * align));
  char *base1 = arena.data() + (align - reinterpret_cast<uintptr_t>(arena.data()) % align) % align;
  char *base2 = base1 + 7 * align;
  ws.bind(base1);
  std::vector<char *> first;
  int64_t prev = -1;
  for (size_t i = 0; i < order.size(); ++i) {
    char *p = held(order[i]);
    first.push_back(p);
    const int64_t off = p - base1;
    CHECK(off == ex.offs[i]);   // the independent running sum
    CHECK(off % align == 0);    // aligned start
    CHECK(off >= prev);         // take order
    CHECK(off <= ws.bytes());
    prev = off;
  }
  // typed destinations really hold typed pointers
  CHECK(reinterpret_cast<char *>(ctx->net[1].h[2]) == base1 + ex.offs[8 + 2]);
  CHECK(reinterpret_cast<char *>(ctx->net[0].w16[1][0]) == base1 + ex.offs[3 + 2]);
  CHECK(static_cast<char *>(ctx->net[0].raw) == base1 + ex.offs[7]);
  CHECK(ctx->bytes == base1 + ex.offs[16]);
  // a second bind moves every pointer by the same amount
  ws.bind(base2);
  for (size_t i = 0; i < order.size(); ++i) CHECK(held(order[i]) - first[i] == base2 - base1);
}

static void check_real_memory() {
  // bind into a real allocation and touch the first and last byte of every buffer (ASan)
  Workspace ws(256, 1024);
  float *a = nullptr;
  uint16_t *b = nullptr;
  char *c = nullptr;
  ws.take_n(&a, 33);      // element counts of the destination's type
  ws.take_n(&b, 129, 0);
  ws.take(&c, 77);
  std::vector<char> arena(static_cast<size_t>(ws.bytes()));
  ws.bind(arena.data());
  a[0] = 1.f, a[32] = 2.f;
  b[0] = 3, b[128] = 4;
  c[0] = 5, c[76] = 6;
  CHECK(reinterpret_cast<char *>(b) - arena.data() == 256 + 1024);
  CHECK(c - arena.data() == 256 + 1024 + 512);
  CHECK(ws.bytes() == 256 + 1024 + 512 + 256 + 1024);
  CHECK(a[32] == 2.f && b[128] == 4 && c[76] == 6);
}

static void check_param_layout() {
  std::vector<int64_t> offs;
  ParamLayout lay{&offs};
  const int64_t counts[] = {6, 64 * 27, 64, 1, 16, 17, 4 * 128 * 128, 3};
  int64_t at = 0;
  std::vector<int64_t> expect;
  for (int64_t n : counts) {
    const int64_t got = lay.add(n);
    expect.push_back(at);
    CHECK(got == at);
    CHECK(got % 16 == 0);
    at = round_up(at + n, 16);
    CHECK(lay.total() == at);
    CHECK(lay.total() % 16 == 0);
  }
  CHECK(offs == expect);  // recorded in call order
  ParamLayout bare;       // no offsets vector: add() still lays out
  CHECK(bare.add(5) == 0 && bare.add(1) == 16 && bare.total() == 32);
}

int main() {
  check_arena(256, 0, 0);       // the CNN / BiLSTM arenas
  check_arena(256, 0, 256);     // the layered arena's spare bytes
  check_arena(256, 1024, 0);    // the wide arena: slack after each buffer, packed images
  check_arena(256, 0, 1024);    // the fused arena's tail
  check_arena(64, 64, 192);
  check_real_memory();
  check_param_layout();
  if (g_failed) std::fprintf(stderr, "%d check(s) failed\n", g_failed);
  return g_failed ? 1 : 0;
}
