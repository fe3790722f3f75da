// Host-side layout planning shared by every engine: the flat parameter layout (ParamLayout) and
// the carve-out of a device arena (Workspace).  A buffer is named once, in the take() line that
// gives its extent; bind() then points every recorded destination into the allocated arena.
// Plain C++ (no HIP header): the allocation itself is workspace_alloc() in common.h.
#pragma once

#include <cstdint>
#include <vector>

namespace ppo {

constexpr int64_t kParamAlign = 16;  // floats: every flat tensor starts 64-B aligned
constexpr int64_t kWsAlign = 256;    // bytes: every workspace buffer starts 256-B aligned

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Flat parameter offsets in torch parameters() order: add() records where a tensor of `count`
// floats starts (in *offsets too, when given) and advances to the next 64-B boundary.
struct ParamLayout {
  std::vector<int64_t> *offsets = nullptr;
  int64_t off = 0;
  int64_t add(int64_t count) {
    const int64_t at = off;
    if (offsets) offsets->push_back(at);
    off = align_up(off + count, kParamAlign);
    return at;
  }
  int64_t total() const { return off; }
};

// One device arena.  Every buffer starts on an `align` boundary and is followed by `slack` spare
// bytes (a take() may override the slack); `tail` spare bytes end the arena.
class Workspace {
 public:
  explicit Workspace(int64_t align, int64_t slack = 0, int64_t tail = 0)
      : align_(align), slack_(slack), tail_(tail) {}

  template <class T>
  void take(T **dst, int64_t bytes, int64_t slack = -1) {
    const int64_t at = align_up(size_, align_);
    slots_.push_back(
        {dst, at, [](void *d, char *p) { *static_cast<T **>(d) = reinterpret_cast<T *>(p); }});
    size_ = align_up(at + bytes, align_) + (slack < 0 ? slack_ : slack);
  }
  // the same for `count` elements of the destination's type
  template <class T>
  void take_n(T **dst, int64_t count, int64_t slack = -1) {
    take(dst, count * static_cast<int64_t>(sizeof(T)), slack);
  }
  int64_t bytes() const { return size_ + tail_; }
  void bind(void *base) const {
    for (const Slot &s : slots_) s.set(s.dst, static_cast<char *>(base) + s.at);
  }

 private:
  struct Slot {
    void *dst;
    int64_t at;
    void (*set)(void *dst, char *p);
  };
  int64_t align_, slack_, tail_, size_ = 0;
  std::vector<Slot> slots_;
};

}  // namespace ppo
