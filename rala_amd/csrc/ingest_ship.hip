// A file's bytes to device memory: reader threads with pinned staging blocks of their own, every block's copy queued behind
// its read, so that the disk / page cache and PCIe work at the same time.
#include <atomic>
#include <mutex>
#include <thread>

#include "ingest_common.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

namespace {

constexpr uint32_t kMaxReaders = 8;        // (measured at C3: 4 readers 107 ms, 8: 70 - 73 ms, 12 - 16: 85 - 130 ms on the 16 CPUs a box allows)

// Pinned staging blocks are expensive to make (the pages are locked one by one) and cheap to keep: a pool of the
// process, two blocks per reader.
struct StagingPool {
    std::mutex m;
    std::vector<void*> free_blocks;
    // (never freed: at process exit the runtime may be gone before this object is, and the memory goes with the process)
    void* take() {
        {
            std::lock_guard<std::mutex> hold(m);
            if (!free_blocks.empty()) { void* p = free_blocks.back(); free_blocks.pop_back(); return p; }
        }
        void* p = nullptr;
        return hipHostMalloc(&p, kBlockBytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    void give(void* p) {
        std::lock_guard<std::mutex> hold(m);
        free_blocks.push_back(p);
    }
};
StagingPool& staging() {
    static StagingPool pool;
    return pool;
}

}  // namespace

int rala_hip::ingest::ship_file(int fd, uint64_t off, uint64_t len, uint8_t* dev, int device, uint32_t threads, const BlockScan* scan,
                                const std::function<bool()>& meanwhile, uint32_t* n_readers_out) {
    const uint64_t n_blocks = (len + kBlockBytes - 1) / kBlockBytes;
    const uint32_t n_readers = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(threads ? threads : 1, kMaxReaders), n_blocks));
    if (n_readers_out) *n_readers_out = n_readers;
    std::atomic<uint64_t> next(0);
    std::atomic<int> failed(0);
    std::vector<std::thread> readers;
    for (uint32_t t = 0; t < n_readers && n_blocks; ++t) {
        readers.emplace_back([&]() {
            if (hipSetDevice(device) != hipSuccess) { failed = 1; return; }
            hipStream_t cs = nullptr;
            hipEvent_t ev[2] = {nullptr, nullptr};
            void* blk[2] = {staging().take(), staging().take()};
            bool ok = blk[0] && blk[1] && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess &&
                      hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
                      hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
            bool busy[2] = {false, false};
            for (int k = 0; ok && !failed; k ^= 1) {
                const uint64_t b = next.fetch_add(1);
                if (b >= n_blocks) break;
                if (busy[k]) ok = hipEventSynchronize(ev[k]) == hipSuccess;       // the block's last copy has left it
                const uint64_t o = b * kBlockBytes;
                const size_t n = (size_t)std::min<uint64_t>(kBlockBytes, len - o);
                size_t got = 0;
                while (ok && got < n) {
                    const ssize_t r = pread(fd, (char*)blk[k] + got, n - got, (off_t)(off + o + got));
                    if (r <= 0) { ok = false; break; }
                    got += (size_t)r;
                }
                if (ok && dev) {
                    ok = hipMemcpyAsync(dev + o, blk[k], n, hipMemcpyHostToDevice, cs) == hipSuccess && hipEventRecord(ev[k], cs) == hipSuccess;
                    busy[k] = ok;
                }
                if (ok && scan) (*scan)(b, (const uint8_t*)blk[k], n);     // (reads the block while it is copied)
            }
            if (cs) ok = (hipStreamSynchronize(cs) == hipSuccess) && ok;
            if (!ok) failed = 1;
            for (int k = 0; k < 2; ++k) {
                if (ev[k]) (void)hipEventDestroy(ev[k]);
                if (blk[k]) staging().give(blk[k]);
            }
            if (cs) (void)hipStreamDestroy(cs);
        });
    }
    const bool room = meanwhile();
    for (auto& th : readers) th.join();
    return !room ? 2 : failed ? 1 : 0;
}
