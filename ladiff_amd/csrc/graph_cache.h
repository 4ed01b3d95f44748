// What the library's two graph users (the sampler: reverse.hip; the decode graph: api.hip) share: the stream a graph is captured on, the
// one capture-and-instantiate sequence, and the rule that decides whether an instantiated graph may still be replayed.
#pragma once
#include <atomic>

#include "common.h"
#include "graph_key.h"

namespace ladiff {

// Graph replay and the round-3 memory fault.  Seen on ROCm 7.2 / MI355X (scripts/repro_seq.py, scripts/repro_graph.py): the graphs of one
// sampler, replayed after two OTHER samplers had instantiated theirs and a blocking hipMemcpy had run in between, faulted at a wild
// address (MEMORY_APERTURE_VIOLATION / an address in the host heap's range), every captured pointer still alive.  Round 4 bisected it
// (profiles/r4/06_*): with the rule below switched off the fault reproduces every time; it goes away when the prologue graph's ONE
// memset node (hipMemsetAsync of the 16-byte step counter) is issued outside the graph, and stays away with every KERNEL node of both
// graphs replayed from the old execs.  So: an older exec's MEMSET NODE is what the runtime replays wrongly after newer instantiations
// - kernel nodes (by-value argument blocks up to 3.8 KB, 300 nodes) are fine, also in a library-free program
// (scripts/repro_graph_args.hip: clean in every configuration, the memset-node case included - the trigger needs more than that
// program has, and was not reduced further).  Fix: NOTHING captured by this library is a memset node any more (launch_zero_fill
// kernels: the step counter in the prologue graph, the ragged decode's output clear); tests/test_gpu_pipeline.py replays old execs on
// purpose (LADIFF_GRAPH_EPOCH_OFF) and gets identical bits.  The rule stays as a second line, cheap (a few hundred microseconds when
// samplers alternate): a graph is replayed only while it is the newest instantiation of THIS library; instantiations by other
// components of the process (torch CUDA graphs, RCCL) do not count - they were never implicated (scripts/repro_graph.py 'graphs').
inline std::atomic<uint64_t> g_graph_epoch{0};
inline std::atomic<int> g_graph_epoch_rule{1};       // ladiff_debug_set_graph_epoch_rule
inline std::atomic<int> g_graph_instantiations{0};   // ladiff_debug_graph_instantiations

// Graphs are CAPTURED on a stream of the handle's own and replayed on the caller's (round 5).  While a stream captures, a
// hipEventQuery of any event that belongs to it is refused and invalidates the capture - and torch.distributed's watchdog thread
// polls the end events of synchronous collectives, which run on the caller's CURRENT stream: a capture on that stream died about
// once in fifteen bench runs under torchrun (profiles/r5/26_*).  Nobody else holds events of this stream.
struct CaptureStream {
    hipStream_t s = nullptr;
    int dev = -1;                         // the device `s` was created on
    // The capture stream belongs to the device that was current when it was created; a handle that is later used with another device
    // current gets a new one (the old graphs hold that device's pointers and are rebuilt by their key anyway).
    int ensure() {
        int cur = 0;
        LADIFF_HIP(hipGetDevice(&cur));
        if (s != nullptr && dev != cur) destroy();
        if (s == nullptr) { LADIFF_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); dev = cur; }
        return 0;
    }
    void destroy() {
        if (s != nullptr) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};

// body(cs) enqueues on `cs` what the graph shall hold; *out receives the instantiated graph.  A failure of the body wins over the
// capture's own error, and the captured graph is destroyed either way.  Every instantiate attempt counts.
template <class Body>
int capture_graph(hipStream_t cs, Body&& body, hipGraphExec_t* out) {
    hipGraph_t graph = nullptr;
    LADIFF_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = body(cs);
    const hipError_t ec = hipStreamEndCapture(cs, &graph);
    if (rc != 0) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    LADIFF_HIP(ec);
    const hipError_t ei = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    ++g_graph_instantiations;
    (void)hipGraphDestroy(graph);
    LADIFF_HIP(ei);
    return 0;
}

// What a handle remembers of its instantiated graphs: the key they were captured for and g_graph_epoch at their instantiation.
struct GraphSlot {
    GraphKey key;
    uint64_t epoch = 0;
    // ladiff_debug_set_graph_epoch_rule(0) (test aid): trust an older exec, as tests/test_gpu_stress.py does to show that the graphs -
    // kernel nodes only since round 4 - replay correctly however old they are.  The switch is process-wide: samplers and decode graphs
    bool newest() const { return epoch == g_graph_epoch.load() || g_graph_epoch_rule.load() == 0; }
    void stamp(const GraphKey& k) { key = k; epoch = ++g_graph_epoch; }
};

}  // namespace ladiff
