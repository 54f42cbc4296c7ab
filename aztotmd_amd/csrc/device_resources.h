// What the engine owns on the device besides its stream (host-only): device memory, pinned read-back blocks, the per-kernel timer.  Each type frees what it
// holds in its destructor; destructors never throw and expect the work that uses the memory to have drained (Engine::release sees to that).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace aztot {

void check_hip(hipError_t e, const char* what);

// device memory that lives as long as the arena: the engine's, the pair lists' (ListStore), each sampler's (Samplers)
class DeviceArena
{
public:
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(DeviceArena&& o) noexcept { release(); blocks_.swap(o.blocks_); return *this; }
    ~DeviceArena() { release(); }
    // n elements (never less than 16 bytes), zero-filled on `stream` if asked
    template <typename T> T* alloc(size_t n, bool zero, hipStream_t stream)
    {
        void* p = nullptr;
        check_hip(hipMalloc(&p, std::max<size_t>(sizeof(T) * n, 16)), "hipMalloc");
        blocks_.push_back(p);
        if (zero) check_hip(hipMemsetAsync(p, 0, sizeof(T) * n, stream), "hipMemsetAsync");
        return (T*)p;
    }
    void release() noexcept
    {
        for (void* p : blocks_) (void)hipFree(p);
        blocks_.clear();
    }

private:
    std::vector<void*> blocks_;
};

// A small block of pinned host memory that device values are copied into without stalling the stream: post copies behind the queued work, mark the
// point behind them, and later ask whether they have landed or wait for them.  Block and event are created on first use.
class PinnedReadback
{
public:
    static constexpr size_t kBytes = 512;
    PinnedReadback() = default;
    PinnedReadback(const PinnedReadback&) = delete;
    ~PinnedReadback()
    {
        if (event_) (void)hipEventDestroy(event_);
        if (host_) (void)hipHostFree(host_);
    }
    void post(const void* dev, size_t bytes, hipStream_t stream, size_t at = 0)
    {
        if (!host_) check_hip(hipHostMalloc(&host_, kBytes, hipHostMallocDefault), "hipHostMalloc");
        check_hip(hipMemcpyAsync((char*)host_ + at, dev, bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    }
    void mark(hipStream_t stream)
    {
        if (!event_) check_hip(hipEventCreateWithFlags(&event_, hipEventDisableTiming), "hipEventCreateWithFlags");
        check_hip(hipEventRecord(event_, stream), "hipEventRecord");
    }
    bool landed() const { return event_ && hipEventQuery(event_) == hipSuccess; }      // (false too when nothing was ever marked)
    void wait() const { check_hip(hipEventSynchronize(event_), "hipEventSynchronize"); }
    // what was copied to offset `at` (valid once landed / waited for, or behind a stream synchronisation)
    template <typename T> const T* as(size_t at = 0) const { return (const T*)((const char*)host_ + at); }

private:
    void* host_ = nullptr;
    hipEvent_t event_ = nullptr;
};

struct KernelTimer
{
    std::string name;
    double ms = 0.0;
    long long calls = 0;
};

// per-kernel timing (options.profile): a pair of events around every launch, read once the stream has drained
class KernelTimers
{
public:
    KernelTimers() = default;
    KernelTimers(const KernelTimers&) = delete;
    ~KernelTimers()
    {
        for (auto& p : pending_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        for (auto e : pool_) (void)hipEventDestroy(e);
    }
    template <typename F> void timed(const char* name, hipStream_t stream, F&& launch)
    {
        auto it = index_.find(name);
        if (it == index_.end())
        {
            it = index_.emplace(name, (int)timers_.size()).first;
            timers_.push_back(KernelTimer{name, 0.0, 0});
        }
        hipEvent_t a = event(), b = event();
        check_hip(hipEventRecord(a, stream), "hipEventRecord");
        launch();
        check_hip(hipEventRecord(b, stream), "hipEventRecord");
        pending_.push_back({it->second, a, b});
        if (pending_.size() > 8192) { check_hip(hipStreamSynchronize(stream), "hipStreamSynchronize"); drain(); }
    }
    // something that happened inside another kernel's launch and has no time of its own (a step opened by the pair kernel of the step before): counted only
    void count(const char* name)
    {
        auto it = index_.find(name);
        if (it == index_.end())
        {
            it = index_.emplace(name, (int)timers_.size()).first;
            timers_.push_back(KernelTimer{name, 0.0, 0});
        }
        timers_[it->second].calls += 1;
    }
    // (the stream has drained) adds the elapsed times of the launches since the last call to the totals
    void drain()
    {
        for (auto& p : pending_)
        {
            float ms = 0.f;
            check_hip(hipEventElapsedTime(&ms, p.a, p.b), "hipEventElapsedTime");
            timers_[p.idx].ms += ms;
            timers_[p.idx].calls += 1;
            pool_.push_back(p.a); pool_.push_back(p.b);
        }
        pending_.clear();
    }
    const std::vector<KernelTimer>& totals() const { return timers_; }
    void reset() { for (auto& t : timers_) { t.ms = 0; t.calls = 0; } }

private:
    struct Pending { int idx; hipEvent_t a, b; };
    hipEvent_t event()
    {
        hipEvent_t e;
        if (!pool_.empty()) { e = pool_.back(); pool_.pop_back(); }
        else check_hip(hipEventCreate(&e), "hipEventCreate");
        return e;
    }
    std::vector<KernelTimer> timers_;
    std::map<std::string, int> index_;
    std::vector<Pending> pending_;
    std::vector<hipEvent_t> pool_;
};

}  // namespace aztot
