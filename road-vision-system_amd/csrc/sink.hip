// Motion-JPEG file sink, the counterpart of capture.hip: one writer thread
// per file over a ring of pinned host slots.  rv_sink_write_batch only records
// an event on the caller's stream (behind the encode that fills the device
// streams) and hands each frame's device address to its writer; it never makes
// the GPU stream wait.  The writer waits for the event, copies the 16-byte
// stream header (rvhip.h, RV_JPEG_STREAM_*) on a stream of its own, then only
// the image's bytes rounded up to 4 KiB, and appends the image to the file, in
// submission order.  A full ring blocks the caller; nothing is dropped
// silently: a frame that overflowed its capacity, a stream that is not one,
// and an I/O error are counted, and the next rv_sink_write_batch and
// rv_sink_close fail with the cause in rv_last_error.
//
// The file is plain Motion-JPEG (complete JPEG images back to back), what
// RV_CAP_MJPEG reads.  No MP4 / AVI muxer: the container carries no timing.
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <errno.h>
#include <string.h>

#include "common.h"

namespace rv {

namespace {

constexpr size_t kCopyRound = 4096;
constexpr size_t kHdr = RV_JPEG_STREAM_HEADER_BYTES;

struct SinkSlot {
  uint8_t* p = nullptr;  // pinned, `capacity` bytes
  hipEvent_t ev = nullptr;
  const uint8_t* dev = nullptr;
  int state = 0;  // 0 free, 1 submitted
};

struct Sink {
  FILE* f = nullptr;
  std::string path;
  int device = 0;
  size_t capacity = 0;
  std::vector<SinkSlot> slots;
  int head = 0, tail = 0;  // next slot to submit / to write
  std::mutex m;
  std::condition_variable cv_submit, cv_free;
  std::thread th;
  hipStream_t copy_stream = nullptr;
  bool stop = false;
  // under the mutex
  int64_t submitted = 0, written = 0, bytes_written = 0, bytes_copied = 0, overflowed = 0,
          io_errors = 0;
  std::string errmsg;  // the first failure not yet reported to the caller
};

void fail_frame(Sink* k, int64_t* counter, const char* fmt, long long frame, const char* what) {
  char msg[512];
  snprintf(msg, sizeof(msg), fmt, k->path.c_str(), frame, what);
  std::lock_guard<std::mutex> lk(k->m);
  ++*counter;
  if (k->errmsg.empty()) k->errmsg = msg;
}

// One submitted slot -> the file.  Runs on the writer thread.
void write_slot(Sink* k, SinkSlot& s, int64_t frame) {
  hipError_t e = hipEventSynchronize(s.ev);
  if (e == hipSuccess) e = hipMemcpyAsync(s.p, s.dev, kHdr, hipMemcpyDeviceToHost, k->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(k->copy_stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    fail_frame(k, &k->io_errors, "%s: frame %lld: %s", frame, hipGetErrorString(e));
    return;
  }
  size_t copied = kHdr;
  uint32_t hdr[4];
  memcpy(hdr, s.p, sizeof(hdr));
  const size_t n = hdr[1];
  if (hdr[0] != RV_JPEG_STREAM_MAGIC || (hdr[2] & RV_JPEG_STREAM_BAD_RECORD) || n < 4) {
    fail_frame(k, &k->io_errors, "%s: frame %lld: %s", frame, "not an encoded JPEG stream");
  } else if ((hdr[2] & RV_JPEG_STREAM_OVERFLOW) || kHdr + n > k->capacity) {
    char what[96];
    snprintf(what, sizeof(what), "image of %zu bytes overflowed the capacity of %zu", n,
             k->capacity);
    fail_frame(k, &k->overflowed, "%s: frame %lld: %s", frame, what);
  } else {
    size_t c = (n + kCopyRound - 1) / kCopyRound * kCopyRound;
    if (kHdr + c > k->capacity) c = k->capacity - kHdr;
    e = hipMemcpyAsync(s.p + kHdr, s.dev + kHdr, c, hipMemcpyDeviceToHost, k->copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(k->copy_stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      fail_frame(k, &k->io_errors, "%s: frame %lld: %s", frame, hipGetErrorString(e));
    } else {
      copied += c;
      if (fwrite(s.p + kHdr, 1, n, k->f) != n) {
        fail_frame(k, &k->io_errors, "%s: frame %lld: write failed: %s", frame, strerror(errno));
      } else {
        std::lock_guard<std::mutex> lk(k->m);
        ++k->written;
        k->bytes_written += (int64_t)n;
      }
    }
  }
  std::lock_guard<std::mutex> lk(k->m);
  k->bytes_copied += (int64_t)copied;
}

void writer_main(Sink* k) {
  (void)hipSetDevice(k->device);
  int64_t frame = 0;
  for (;;) {
    int i;
    {
      std::unique_lock<std::mutex> lk(k->m);
      k->cv_submit.wait(lk, [&] { return k->stop || k->slots[k->tail].state == 1; });
      if (k->slots[k->tail].state != 1) return;  // stop, and every submitted frame is written
      i = k->tail;
    }
    write_slot(k, k->slots[i], frame++);
    {
      std::lock_guard<std::mutex> lk(k->m);
      k->slots[i].state = 0;
      k->tail = (k->tail + 1) % (int)k->slots.size();
    }
    k->cv_free.notify_all();
  }
}

// The first unreported failure -> rv_last_error; true when there was one.
bool report_pending(Sink* k) {
  std::lock_guard<std::mutex> lk(k->m);
  if (k->errmsg.empty()) return false;
  set_error("%s", k->errmsg.c_str());
  k->errmsg.clear();
  return true;
}

void destroy(Sink* k) {
  for (auto& s : k->slots) {
    if (s.ev) (void)hipEventDestroy(s.ev);
    if (s.p) (void)hipHostFree(s.p);
  }
  if (k->copy_stream) (void)hipStreamDestroy(k->copy_stream);
  if (k->f) fclose(k->f);
  delete k;
}

}  // namespace

extern "C" int rv_sink_open(const char* path, int nbuf, size_t capacity, void** handle) {
  RV_CHECK_ARG(path != nullptr && handle != nullptr, "null pointer");
  RV_CHECK_ARG(nbuf >= 2 && nbuf <= 64, "nbuf %d out of [2, 64]", nbuf);
  RV_CHECK_ARG(capacity >= 1024 && capacity <= ((size_t)1 << 31), "sink capacity %zu", capacity);
  *handle = nullptr;
  Sink* k = new Sink();
  k->path = path;
  k->capacity = capacity;
  int rc = hip_check(hipGetDevice(&k->device), "hipGetDevice(sink)");
  if (rc == RV_OK)
    rc = hip_check(hipStreamCreateWithFlags(&k->copy_stream, hipStreamNonBlocking),
                   "hipStreamCreate(sink)");
  k->slots.resize(nbuf);
  for (auto& s : k->slots) {
    void* p = nullptr;
    if (rc == RV_OK) rc = hip_check(hipHostMalloc(&p, capacity, hipHostMallocDefault), "hipHostMalloc(sink)");
    s.p = (uint8_t*)p;
    if (rc == RV_OK)
      rc = hip_check(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming), "hipEventCreate(sink)");
  }
  if (rc == RV_OK) {
    k->f = fopen(path, "wb");
    if (!k->f) {
      set_error("cannot create %s: %s", path, strerror(errno));
      rc = RV_EINVAL;
    }
  }
  if (rc != RV_OK) {
    destroy(k);
    return rc;
  }
  k->th = std::thread(writer_main, k);
  *handle = k;
  return RV_OK;
}

extern "C" int rv_sink_write_batch(void* const* handles, int S, const uint8_t* streams,
                                   size_t stream_stride, void* stream) {
  RV_CHECK_ARG(handles != nullptr && streams != nullptr && S >= 1, "bad arguments");
  for (int s = 0; s < S; ++s) {
    Sink* k = static_cast<Sink*>(handles[s]);
    RV_CHECK_ARG(k != nullptr && stream_stride >= k->capacity,
                 "stream %d: null handle, or a stride below the sink's capacity", s);
  }
  for (int s = 0; s < S; ++s)
    if (report_pending(static_cast<Sink*>(handles[s]))) return RV_EINVAL;
  for (int s = 0; s < S; ++s) {
    Sink* k = static_cast<Sink*>(handles[s]);
    int i;
    {
      std::unique_lock<std::mutex> lk(k->m);  // a full ring blocks the caller
      k->cv_free.wait(lk, [&] { return k->slots[k->head].state == 0; });
      i = k->head;
    }
    SinkSlot& sl = k->slots[i];
    const int rc = hip_check(hipEventRecord(sl.ev, as_stream(stream)), "hipEventRecord(sink)");
    if (rc != RV_OK) return rc;
    sl.dev = streams + (size_t)s * stream_stride;
    {
      std::lock_guard<std::mutex> lk(k->m);
      sl.state = 1;
      k->head = (k->head + 1) % (int)k->slots.size();
      ++k->submitted;
    }
    k->cv_submit.notify_one();
  }
  return RV_OK;
}

extern "C" int rv_sink_stats(void* handle, int64_t* stats) {
  RV_CHECK_ARG(handle != nullptr && stats != nullptr, "null pointer");
  Sink* k = static_cast<Sink*>(handle);
  std::lock_guard<std::mutex> lk(k->m);
  stats[0] = k->submitted;
  stats[1] = k->written;
  stats[2] = k->bytes_written;
  stats[3] = k->bytes_copied;
  stats[4] = k->overflowed;
  stats[5] = k->io_errors;
  stats[6] = (int64_t)k->slots.size();
  stats[7] = (int64_t)k->capacity;
  return RV_OK;
}

extern "C" int rv_sink_flush(void* handle) {
  RV_CHECK_ARG(handle != nullptr, "null pointer");
  Sink* k = static_cast<Sink*>(handle);
  {
    std::unique_lock<std::mutex> lk(k->m);
    k->cv_free.wait(lk, [&] {
      for (auto& s : k->slots)
        if (s.state != 0) return false;
      return true;
    });
  }
  if (fflush(k->f) != 0) {
    set_error("%s: flush failed: %s", k->path.c_str(), strerror(errno));
    return RV_EINVAL;
  }
  return report_pending(k) ? RV_EINVAL : RV_OK;
}

extern "C" int rv_sink_close(void* handle) {
  if (!handle) return RV_OK;
  Sink* k = static_cast<Sink*>(handle);
  {
    std::lock_guard<std::mutex> lk(k->m);
    k->stop = true;  // the writer leaves once every submitted frame is written
  }
  k->cv_submit.notify_all();
  if (k->th.joinable()) k->th.join();
  int rc = RV_OK;
  if (fflush(k->f) != 0) {
    set_error("%s: flush failed: %s", k->path.c_str(), strerror(errno));
    rc = RV_EINVAL;
  }
  if (report_pending(k)) rc = RV_EINVAL;
  destroy(k);
  return rc;
}

}  // namespace rv
