// Captured hipGraphs of whole stage calls: the capture primitive every stage uses, and the cached exec on top of it
// (FaCodec decode and encode, prior stack, prompt encoders; the PVA flow keeps a cache of its own around capture_exec).
#pragma once
#include "common.hpp"

namespace fl {

// Captures body(cap) on `cap` and instantiates the graph into *exec.  A body error ends the capture, drops the graph and
// is returned as it is.  A fork onto further streams and the join back belong inside the body.
template <class F>
static int capture_exec(hipStream_t cap, hipGraphExec_t* exec, F&& body) {
  FL_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed));
  const int r = body(cap);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(cap, &g);
  if (r) {
    if (g) (void)hipGraphDestroy(g);
    return r;
  }
  FL_HIP(e);
  const hipError_t ie = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  FL_HIP(ie);
  return kOk;
}

// One cached hipGraph of a whole stage call, re-captured when the call's key (pointers, shapes) changes.
struct CapGraph {
  hipGraphExec_t exec = nullptr;
  hipStream_t cap = nullptr;
  std::vector<const void*> key;
  void retire() {  // the exec only: the next call captures again
    retire_graph(exec);
    key.clear();
  }
  void release() {
    retire_graph(exec);
    if (cap) (void)hipStreamDestroy(cap);
    *this = CapGraph();
  }
};

template <class F>
static int with_graph(CapGraph& g, const std::vector<const void*>& key_in, bool use_graph, hipStream_t st, F&& body) {
  if (!use_graph) return body(st);
  // the captured launches bake in the knobs the body read: the process tune epoch is part of the key
  std::vector<const void*> key = key_in;
  key.push_back((const void*)(intptr_t)tune_epoch());
  if (!g.exec || g.key != key) {
    retire_graph(g.exec);
    if (!g.cap) FL_HIP(hipStreamCreateWithFlags(&g.cap, hipStreamNonBlocking));
    const int r = capture_exec(g.cap, &g.exec, body);
    if (r) return r;
    g.key = key;
  }
  FL_HIP(hipGraphLaunch(g.exec, st));
  note_graph_use(g.exec, st);
  return kOk;
}

}  // namespace fl
