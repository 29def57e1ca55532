// shc_stage.hpp — how a host array reaches a kernel and a kernel's result reaches a host array: one arena over the engine's staging buffer, one scope per call.
//
// StageArena hands out bytes of the engine's persistent staging allocation with stack discipline.  HostCall is the scope of one entry point: it records the
// arena's mark, gives typed device views of the caller's arrays (in / out / in2d / out2d) and device bytes of its own (scratch), and on destruction releases
// what it took.  One memory rule: take from the arena; a request that does not fit becomes a temporary device allocation the scope owns.  An entry point
// that calls another entry point while its own staged data is live is safe by construction: the inner scope carves above the outer one's bytes.
//
// Included twice by shc_engine.hip: before struct shc_engine for the arena it owns (plain host C++, no HIP: tests/stage_arena_check.cpp compiles this part
// alone with SHC_STAGE_ARENA_ONLY), and once the engine is complete for the scope.
#ifndef SHC_STAGE_ARENA
#define SHC_STAGE_ARENA

#include <cstddef>
#include <cstdint>

struct StageArena {
  static constexpr size_t npos = ~size_t(0); // "does not fit": the cursor stays where it was
  char *base;
  size_t capacity, cursor;
  // the offset of `bytes` bytes whose ADDRESS is a multiple of `align` (a power of two), or npos
  size_t take(size_t bytes, size_t align) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    const size_t pad = size_t((align - (b + cursor) % align) % align);
    if (pad > capacity - cursor || bytes > capacity - cursor - pad) return npos;
    const size_t at = cursor + pad;
    cursor = at + bytes;
    return at;
  }
  // ... of `count` elements of `size` bytes (a product that overflows does not fit)
  size_t take(size_t count, size_t size, size_t align) { return size && count > npos / size ? npos : take(count * size, align); }
  size_t mark() const { return cursor; }
  void release(size_t mark) { cursor = mark; }
};

#elif !defined(SHC_STAGE_ARENA_ONLY) // ----------------------------------------------------------- the per-call scope (struct shc_engine is complete)

struct HostCall {
  static constexpr size_t kAlign = 16; // every view: the widest access of the kernels that read staged data (double2)
  struct CopyBack {
    void *dst;
    const void *src;
    size_t bytes, pitch, rows; // rows != 0: `rows` rows of `bytes` bytes, `pitch` bytes apart at the host
  };
  StageArena &arena;
  hipStream_t stream;
  size_t mark;
  hipError_t err = hipSuccess;
  const char *what = "";
  bool live = false; // the stream may still read or write bytes of this scope, or a caller's host array
  std::vector<void *> temps;
  std::vector<CopyBack> backs;

  explicit HostCall(shc_engine *e) : HostCall(e->stage, e->stream) {}
  HostCall(StageArena &a, hipStream_t s) : arena(a), stream(s), mark(a.mark()) {} // (a call without an engine: an empty arena of its own, temporaries only)
  HostCall(const HostCall &) = delete;
  HostCall &operator=(const HostCall &) = delete;
  ~HostCall() {
    if (live) (void)hipStreamSynchronize(stream); // left without finish(): no kernel may still read what is released below
    for (void *t : temps) (void)hipFree(t);
    arena.release(mark);
  }
  bool check(hipError_t r, const char *op) {
    if (err == hipSuccess && r != hipSuccess) err = r, what = op;
    return err == hipSuccess;
  }
  int status() const { return err == hipSuccess ? SHC_OK : fail(SHC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err)); }

  void wait_at_finish() { live = true; } // a launch that the caller must see completed although nothing was staged for it
  // device bytes that live as long as the scope
  template <class T>
  T *scratch(size_t count) {
    if (err != hipSuccess) return nullptr;
    live = true;
    const size_t at = arena.take(count, sizeof(T), kAlign);
    if (at != StageArena::npos) return reinterpret_cast<T *>(arena.base + at);
    void *t = nullptr;
    if (count > StageArena::npos / sizeof(T)) check(hipErrorOutOfMemory, "staging request");
    else if (check(hipMalloc(&t, count * sizeof(T)), "hipMalloc (staging temporary)")) temps.push_back(t);
    return static_cast<T *>(t);
  }
  // a copy of `count` elements at device address `d` into the host array `dst`, enqueued by finish()
  template <class T>
  void back(T *dst, const T *d, size_t count) {
    if (dst && d && count) backs.push_back(CopyBack{dst, d, count * sizeof(T), 0, 0});
  }
  // device view of an input array: the caller's pointer, or staged bytes and a copy on the stream
  template <class T>
  const T *in(const T *src, size_t count, int on_device) {
    if (!src || on_device || !count) return src;
    T *d = scratch<T>(count);
    if (d) check(hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, stream), "hipMemcpyAsync (host to device)");
    return err == hipSuccess ? d : nullptr;
  }
  // device pointer for an output: the caller's pointer, or staged bytes that finish() copies back
  template <class T>
  T *out(T *dst, size_t count, int on_device) {
    if (!dst || on_device || !count) return dst;
    T *d = scratch<T>(count);
    back(dst, d, count);
    return d;
  }
  // ... of a host array whose rows of `width` bytes lie `pitch` bytes apart: dense rows on the device
  char *in2d(const void *src, size_t width, size_t pitch, size_t rows) {
    char *d = rows && width <= StageArena::npos / rows ? scratch<char>(rows * width) : nullptr;
    if (d) check(hipMemcpy2DAsync(d, width, src, pitch, width, rows, hipMemcpyHostToDevice, stream), "hipMemcpy2DAsync (host to device)");
    return err == hipSuccess ? d : nullptr;
  }
  char *out2d(void *dst, size_t width, size_t pitch, size_t rows) {
    char *d = rows && width <= StageArena::npos / rows ? scratch<char>(rows * width) : nullptr;
    if (d) backs.push_back(CopyBack{dst, d, width, pitch, rows});
    return d;
  }
  // after the kernels: the registered copies, and a wait if the scope staged or returns anything (device pointers only: nothing is enqueued or waited for)
  int finish() {
    check(hipGetLastError(), "kernel launch");
    for (const CopyBack &b : backs) {
      if (b.rows) check(hipMemcpy2DAsync(b.dst, b.pitch, b.src, b.bytes, b.bytes, b.rows, hipMemcpyDeviceToHost, stream), "hipMemcpy2DAsync (device to host)");
      else check(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync (device to host)");
      if (err != hipSuccess) break;
    }
    backs.clear();
    if (live && err == hipSuccess && check(hipStreamSynchronize(stream), "hipStreamSynchronize")) live = false;
    return status();
  }
};

#endif
