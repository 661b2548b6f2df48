// pybind11 bindings for the ddp_amd native extension.
// Tensors cross the boundary as raw device addresses (uintptr_t) plus explicit shapes; the
// Python wrappers in ops/ validate dtype / shape / contiguity / device before calling. Every
// launcher takes the HIP stream explicitly so the calls can be captured into a hipGraph.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "runtime/comm.h"

namespace py = pybind11;
using ddp_amd::BucketSpec;
using ddp_amd::RcclComm;
using ddp_amd::Reducer;

#include "kernels/api.h"

template <typename T>
static T* P(uintptr_t v) { return reinterpret_cast<T*>(v); }
static hipStream_t S(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }
static void check(int rc, const char* what) {
  if (rc != 0) {
    std::string msg = std::string(what) + " failed: ";
    msg += (rc > 0) ? hipGetErrorString((hipError_t)rc) : "invalid arguments";
    throw std::runtime_error(msg);
  }
}

// Cross-stream ordering edge with a DEVICE-scope release: record on `from`, wait on `to`.
// torch.cuda.Stream.wait_stream uses a default event, whose record is a system-scope release
// (an L2 write-back of everything dirty) — measured ~15 us per edge between graph segments.
// Both streams are on this GPU (and RCCL fences its own peer traffic), so device scope suffices.
struct StreamLink {
  hipEvent_t ev = nullptr;
  StreamLink() {
    check((int)hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventReleaseToDevice),
          "hipEventCreateWithFlags");
  }
  ~StreamLink() {
    if (ev) (void)hipEventDestroy(ev);
  }
  void link(uintptr_t from, uintptr_t to) {
    check((int)hipEventRecord(ev, S(from)), "hipEventRecord");
    check((int)hipStreamWaitEvent(S(to), ev, 0), "hipStreamWaitEvent");
  }
  void record(uintptr_t s) { check((int)hipEventRecord(ev, S(s)), "hipEventRecord"); }
  void wait(uintptr_t s) { check((int)hipStreamWaitEvent(S(s), ev, 0), "hipStreamWaitEvent"); }
};

// (z, coef, sums, pool, relu, Hz, Wz) -> BnBwdFuse (None -> nullptr)
static const ddp_amd::BnBwdFuse* bn_fuse(py::object o, ddp_amd::BnBwdFuse* f) {
  if (o.is_none()) return nullptr;
  auto t = o.cast<py::tuple>();
  f->z = P<unsigned short>(t[0].cast<uintptr_t>());
  f->coef = P<float>(t[1].cast<uintptr_t>());
  f->sums = P<float>(t[2].cast<uintptr_t>());
  f->pool = t[3].cast<int>();
  f->relu = t[4].cast<int>();
  f->Hz = t[5].cast<int>();
  f->Wz = t[6].cast<int>();
  f->code = t.size() > 7 ? P<unsigned>(t[7].cast<uintptr_t>()) : nullptr;
  return f;
}

// (dz, dgamma, dbeta) -> BnBwdApply (None -> nullptr)
static const ddp_amd::BnBwdApply* bn_apply(py::object o, ddp_amd::BnBwdApply* out) {
  if (o.is_none()) return nullptr;
  auto t = o.cast<py::tuple>();
  out->dz = P<unsigned short>(t[0].cast<uintptr_t>());
  out->dgamma = P<float>(t[1].cast<uintptr_t>());
  out->dbeta = P<float>(t[2].cast<uintptr_t>());
  return out;
}

// (smoothing, partner labels | 0, lam | 0)
static ddp_amd::SoftTarget soft_target(py::object o) {
  auto t = o.cast<py::tuple>();
  if (t.size() != 3) throw std::runtime_error("soft target needs (smoothing, labels_b, lam)");
  return {t[0].cast<float>(), P<long long>(t[1].cast<uintptr_t>()),
          P<float>(t[2].cast<uintptr_t>())};
}

static ddp_amd::ConvGeom geom(py::tuple g) {
  if (g.size() != 12 && g.size() != 13) throw std::runtime_error("conv geometry needs 12/13 ints");
  ddp_amd::ConvGeom c;
  c.wkrsc = 0;
  int* f = &c.N;
  for (size_t i = 0; i < g.size(); ++i) f[i] = g[i].cast<int>();
  return c;
}

// conv weight pack descriptors from Python: (p, wc, wt, K, Cr, C, R, S, krsc) each
using PackTuple = std::tuple<uintptr_t, uintptr_t, uintptr_t, int, int, int, int, int, int>;
static std::vector<ddp_amd::PackDesc> pack_descs(const std::vector<PackTuple>& descs) {
  std::vector<ddp_amd::PackDesc> d;
  for (const auto& [p, wc, wt, k, cr, c, r, s, krsc] : descs)
    d.push_back({P<float>(p), P<unsigned short>(wc), P<unsigned short>(wt), k, cr, c, r, s, krsc});
  return d;
}

PYBIND11_MODULE(_native, m) {
  m.doc() = "ddp_amd native extension: gfx950 HIP kernels + RCCL runtime";

  // geometry tuple: (N,H,W,C,K,R,S,stride,pad,P,Q,Creal[,wkrsc])
  // ws / ws_elems: fp32 split-K slab workspace (0 disables split-K); splits 0 = automatic
  m.def("conv_fwd", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, uintptr_t y,
                       uintptr_t stats, uintptr_t ws, size_t ws_elems, int splits, uintptr_t st) {
    auto c = geom(g);
    check(ddp_conv_fwd(&c, P<void>(x), P<void>(wc), P<float>(bias), P<void>(y), P<float>(stats),
                       P<float>(ws), ws_elems, splits, S(st)), "conv_fwd");
  });
  // conv_fwd + the BatchNorm(+ReLU, +2x2 pool) forward fused into its split-K finish when the
  // GEMM is small (api.h BnFwdFuse); bn = (gamma, beta, eps, relu, pool, coef, y, P, Q).
  // Returns True when fused (y and coef written), False when the caller must run bn_act_fwd.
  m.def("conv_fwd_bn", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, uintptr_t z,
                          uintptr_t stats, uintptr_t ws, size_t ws_elems, uintptr_t st,
                          py::tuple bn) {
    auto c = geom(g);
    ddp_amd::BnFwdFuse f{};
    f.gamma = P<float>(bn[0].cast<uintptr_t>());
    f.beta = P<float>(bn[1].cast<uintptr_t>());
    f.eps = bn[2].cast<float>();
    f.relu = bn[3].cast<int>();
    f.pool = bn[4].cast<int>();
    f.coef = P<float>(bn[5].cast<uintptr_t>());
    f.y = P<unsigned short>(bn[6].cast<uintptr_t>());
    f.P = bn[7].cast<int>();
    f.Q = bn[8].cast<int>();
    const int rc = ddp_conv_fwd_bn(&c, P<void>(x), P<void>(wc), P<float>(bias), P<void>(z),
                                   P<float>(stats), P<float>(ws), ws_elems, &f, S(st));
    if (rc < 0) check(rc, "conv_fwd_bn");
    if (rc >= 2) check(rc - 2, "conv_fwd_bn");
    return rc == 1;
  });
  m.def("conv_bn_fuse_rows", [](int rows) { ddp_conv_bn_fuse_rows(rows); });
  // tap-reuse 3x3 forward (conv_tr.hip): returns 0 not served, 1 served, 2 served with the
  // BatchNorm forward fused into its split-K finish (bn = conv_fwd_bn's tuple, or None)
  m.def("conv_fwd_tr", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, uintptr_t z,
                          uintptr_t stats, uintptr_t ws, size_t ws_elems, uintptr_t st,
                          py::object bn, py::object fin) {
    auto c = geom(g);
    ddp_amd::BnFwdFuse f{};
    const ddp_amd::BnFwdFuse* fp = nullptr;
    if (!bn.is_none()) {
      py::tuple b = bn.cast<py::tuple>();
      f.gamma = P<float>(b[0].cast<uintptr_t>());
      f.beta = P<float>(b[1].cast<uintptr_t>());
      f.eps = b[2].cast<float>();
      f.relu = b[3].cast<int>();
      f.pool = b[4].cast<int>();
      f.coef = P<float>(b[5].cast<uintptr_t>());
      f.y = P<unsigned short>(b[6].cast<uintptr_t>());
      f.P = b[7].cast<int>();
      f.Q = b[8].cast<int>();
      fp = &f;
    }
    // fused input (the preceding block's BN + ReLU [+ pool]): (z, stats, gamma, beta, eps,
    // relu, pool, coef, y)
    ddp_amd::TrFwdIn ti{};
    const ddp_amd::TrFwdIn* tp = nullptr;
    if (!fin.is_none()) {
      py::tuple b = fin.cast<py::tuple>();
      ti.z = P<unsigned short>(b[0].cast<uintptr_t>());
      ti.stats = P<float>(b[1].cast<uintptr_t>());
      ti.gamma = P<float>(b[2].cast<uintptr_t>());
      ti.beta = P<float>(b[3].cast<uintptr_t>());
      ti.eps = b[4].cast<float>();
      ti.relu = b[5].cast<int>();
      ti.pool = b[6].cast<int>();
      ti.coef = P<float>(b[7].cast<uintptr_t>());
      ti.y = P<unsigned short>(b[8].cast<uintptr_t>());
      tp = &ti;
    }
    int done = 0;
    const int rc = ddp_conv_fwd_tr(&c, P<void>(x), P<void>(wc), P<float>(bias), P<void>(z),
                                   P<float>(stats), P<float>(ws), ws_elems, fp, &done, tp, S(st));
    if (rc < 0) check(rc, "conv_fwd_tr");
    if (rc >= 2) check(rc - 2, "conv_fwd_tr");
    return rc == 1 ? 1 + done : 0;
  }, py::arg("g"), py::arg("x"), py::arg("wc"), py::arg("bias"), py::arg("z"), py::arg("stats"),
     py::arg("ws"), py::arg("ws_elems"), py::arg("st"), py::arg("bn") = py::none(),
     py::arg("fin") = py::none());
  // VGG input block with z recomputed (conv_l0.hip): forward = statistics + BN/ReLU/pool
  // passes into y; backward = BN-backward sums + dz passes (dgamma / dbeta accumulated)
  m.def("l0_ok", [](py::tuple g) {
    auto c = geom(g);
    return ddp_l0_ok(&c) == 1;
  });
  m.def("l0_fwd", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, float eps, int relu,
                     uintptr_t stats, uintptr_t gamma, uintptr_t beta, uintptr_t coef, uintptr_t y,
                     uintptr_t code, uintptr_t zw, uintptr_t st) {
    auto c = geom(g);
    ddp_amd::L0Io io{};
    io.zw = P<void>(zw);
    io.x = P<void>(x); io.wc = P<void>(wc); io.bias = P<float>(bias); io.eps = eps; io.relu = relu;
    io.stats = P<float>(stats); io.gamma = P<float>(gamma); io.beta = P<float>(beta);
    io.coef = P<float>(coef); io.y = P<void>(y); io.code = P<void>(code);
    check(ddp_l0_fwd(&c, &io, S(st)), "l0_fwd");
  });
  m.def("l0_bwd", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, float eps, int relu,
                     uintptr_t coef, uintptr_t dy, uintptr_t sums, uintptr_t dz, uintptr_t dgamma,
                     uintptr_t dbeta, uintptr_t code, uintptr_t zw, uintptr_t st, int sums_ready,
                     uintptr_t dw, uintptr_t ws, size_t ws_elems) {
    // dz = 0 with dw / ws: the weight gradient fused into the dz pass (dz never stored).
    // Returns 1 when that form does not serve the call (nothing launched), else 0.
    auto c = geom(g);
    ddp_amd::L0Io io{};
    io.x = P<void>(x); io.wc = P<void>(wc); io.bias = P<float>(bias); io.eps = eps; io.relu = relu;
    io.coef = P<float>(coef); io.dy = P<void>(dy); io.sums = P<float>(sums); io.dz = P<void>(dz);
    io.dgamma = P<float>(dgamma); io.dbeta = P<float>(dbeta); io.code = P<void>(code);
    io.zw = P<void>(zw);
    io.sums_ready = sums_ready;
    io.dw = P<float>(dw); io.ws = P<float>(ws); io.ws_elems = ws_elems;
    const int rc = ddp_l0_bwd(&c, &io, S(st));
    if (rc == -2) return 1;
    check(rc, "l0_bwd");
    return 0;
  }, py::arg("g"), py::arg("x"), py::arg("wc"), py::arg("bias"), py::arg("eps"), py::arg("relu"),
     py::arg("coef"), py::arg("dy"), py::arg("sums"), py::arg("dz"), py::arg("dgamma"),
     py::arg("dbeta"), py::arg("code"), py::arg("zw"), py::arg("stream"),
     py::arg("sums_ready") = 0, py::arg("dw") = 0, py::arg("ws") = 0, py::arg("ws_elems") = 0);
  m.def("conv_tr_would_serve", [](py::tuple g, size_t ws_elems, int in_mode) {
    auto c = geom(g);
    return ddp_conv_tr_would_serve(&c, ws_elems, in_mode) == 1;
  });
  m.def("conv_tr_set", [](int mode, int M, int K, int C, int H, int bm, int bn, int splits,
                          int stages) { ddp_conv_tr_set(mode, M, K, C, H, bm, bn, splits, stages); },
        py::arg("mode"), py::arg("M"), py::arg("K"), py::arg("C"), py::arg("H"), py::arg("bm"),
        py::arg("bn"), py::arg("splits"), py::arg("stages") = 0);
  m.def("conv_tr_geometry", [](int BM, int N, int H, int W) {
    int o[7];
    ddp_conv_tr_geometry(BM, N, H, W, o);
    return std::vector<int>(o, o + 7);
  });
  // the whole head backward (dx fused with the preceding block's BatchNorm backward + dW / db)
  // in one launch; bn = (z, coef, sums, pool, relu, Hz, Wz), bna = (dz, dgamma, dbeta); returns
  // False when not served (nothing launched; dx is then computed by linear_bwd)
  m.def("linear_head_bwd_bn", [](uintptr_t dl, uintptr_t W, uintptr_t x, int B, int F, int J,
                                 uintptr_t g, py::tuple bn, py::tuple bna, uintptr_t dW,
                                 uintptr_t db, uintptr_t st) {
    ddp_amd::BnBwdFuse f{};
    f.z = P<unsigned short>(bn[0].cast<uintptr_t>());
    f.coef = P<float>(bn[1].cast<uintptr_t>());
    f.sums = P<float>(bn[2].cast<uintptr_t>());
    f.pool = bn[3].cast<int>();
    f.relu = bn[4].cast<int>();
    f.Hz = bn[5].cast<int>();
    f.Wz = bn[6].cast<int>();
    ddp_amd::BnBwdApply ap{};
    bn_apply(bna, &ap);
    const int rc = ddp_linear_head_bwd_bn(P<float>(dl), P<float>(W), P<void>(x), B, F, J,
                                          P<float>(g), &f, &ap, P<float>(dW), P<float>(db), S(st));
    if (rc < 0) check(rc, "linear_head_bwd_bn");
    if (rc >= 2) check(rc - 2, "linear_head_bwd_bn");
    return rc == 1;
  });
  // direct MFMA conv for C = 8 input layers; returns False when the shape is not served
  m.def("conv_fwd_smallk", [](py::tuple g, uintptr_t x, uintptr_t wc, uintptr_t bias, uintptr_t y,
                              uintptr_t stats, uintptr_t st) {
    auto c = geom(g);
    const int rc = ddp_conv_fwd_smallk(&c, P<void>(x), P<void>(wc), P<float>(bias), P<void>(y),
                                       P<float>(stats), S(st));
    if (rc > 0) check(rc, "conv_fwd_smallk");
    return rc == 0;
  });
  // bn: optional (z, coef, sums, pool, relu, Hz, Wz) of the preceding Conv->BN->ReLU(->pool)
  // block whose BatchNorm-backward sums the dgrad epilogue accumulates (api.h BnBwdFuse)
  // bna: optional (dz, dgamma, dbeta) — complete that block's BN backward in the split-K finish
  // when possible (api.h BnBwdApply); returns True when it did (dx is then NOT written)
  m.def("conv_dgrad", [](py::tuple g, uintptr_t dy, uintptr_t wt, uintptr_t dx, uintptr_t ws,
                         size_t ws_elems, int splits, uintptr_t st, int accumulate, py::object bn,
                         py::object bna, uintptr_t acc_dy, uintptr_t acc_mask) {
    auto c = geom(g);
    if (acc_mask) {  // accumulate onto a deferred first branch (acc_dy through the ReLU bits)
      check(ddp_conv_dgrad_acc(&c, P<void>(dy), P<void>(wt), P<void>(dx), P<float>(ws), ws_elems,
                               splits, P<void>(acc_dy), P<unsigned char>(acc_mask), S(st)),
            "conv_dgrad_acc");
      return false;
    }
    if (bn.is_none()) {
      check(ddp_conv_dgrad(&c, P<void>(dy), P<void>(wt), P<void>(dx), P<float>(ws), ws_elems,
                           splits, accumulate, S(st)), "conv_dgrad");
      return false;
    }
    ddp_amd::BnBwdFuse f{};
    const ddp_amd::BnBwdFuse* fp = bn_fuse(bn, &f);
    ddp_amd::BnBwdApply ap{};
    const ddp_amd::BnBwdApply* app = bn_apply(bna, &ap);
    int done = 0;
    check(ddp_conv_dgrad_bn(&c, P<void>(dy), P<void>(wt), P<void>(dx), P<float>(ws), ws_elems,
                            splits, fp, app, &done, S(st)), "conv_dgrad_bn");
    return done == 1;
  }, py::arg("g"), py::arg("dy"), py::arg("wt"), py::arg("dx"), py::arg("ws"),
     py::arg("ws_elems"), py::arg("splits"), py::arg("stream"), py::arg("accumulate") = 0,
     py::arg("bn") = py::none(), py::arg("bna") = py::none(), py::arg("acc_dy") = 0,
     py::arg("acc_mask") = 0);
  // one layer's backward: WGRAD (dw += ...) and stride-1 DGRAD (dx = ..., optional BN-backward
  // sums) as one grouped launch when the policy allows (ddp_conv_bwd_pair), else two
  m.def("conv_bwd_pair", [](py::tuple g, uintptr_t dy, uintptr_t wc, uintptr_t dx, uintptr_t x,
                            uintptr_t dw, uintptr_t ws, size_t ws_elems, uintptr_t st,
                            py::object bn, py::object bna) {
    auto c = geom(g);
    ddp_amd::BnBwdApply ap{};
    const ddp_amd::BnBwdApply* app = bn_apply(bna, &ap);
    int done = 0;
    ddp_amd::BnBwdFuse f{};
    const ddp_amd::BnBwdFuse* fp = bn_fuse(bn, &f);
    check(ddp_conv_bwd_pair(&c, P<void>(dy), P<void>(wc), P<void>(dx), P<void>(x), P<float>(dw),
                            P<float>(ws), ws_elems, fp, app, &done, S(st)), "conv_bwd_pair");
    // 1: the preceding block's whole BN backward ran in the finish (bna); 2: the input block's
    // BN-backward sums were taken in the finish (bn with code); 0: neither
    return done;
  }, py::arg("g"), py::arg("dy"), py::arg("wc"), py::arg("dx"), py::arg("x"), py::arg("dw"),
     py::arg("ws"), py::arg("ws_elems"), py::arg("stream"), py::arg("bn") = py::none(),
     py::arg("bna") = py::none());
  // SGD in the backward (world 1): register a conv weight's gradient view with its update
  // (p, momentum buffer, bf16 copy, lr, momentum, wd, grad_scale, nesterov; sched = device
  // learning-rate table used instead of lr, api.h LrSched); dw = 0 with
  // clear = 1 switches it off. sgd_fuse_taken: gradient views whose WGRAD finish applied it
  // since sgd_fuse_begin.
  m.def("sgd_fuse_register", [](uintptr_t dw, uintptr_t p, uintptr_t buf, uintptr_t wc, float lr,
                                float momentum, float wd, float grad_scale, int nesterov,
                                int clear, uintptr_t sched) {
    ddp_amd::SgdFuse f{P<float>(p), P<float>(buf), P<unsigned short>(wc), lr, momentum, wd,
                       grad_scale, nesterov, P<const ddp_amd::LrSched>(sched)};
    ddp_sgd_fuse_register(P<float>(dw), dw ? &f : nullptr, clear);
  }, py::arg("dw"), py::arg("p") = 0, py::arg("buf") = 0, py::arg("wc") = 0, py::arg("lr") = 0.f,
     py::arg("momentum") = 0.f, py::arg("wd") = 0.f, py::arg("grad_scale") = 1.f,
     py::arg("nesterov") = 0, py::arg("clear") = 0, py::arg("sched") = 0);
  m.def("sgd_fuse_begin", []() { ddp_sgd_fuse_begin(); });
  m.def("sgd_fuse_taken", []() {
    std::vector<uintptr_t> v(256);
    int n = ddp_sgd_fuse_taken(v.data(), (int)v.size());
    if (n > (int)v.size()) {
      v.resize(n);
      n = ddp_sgd_fuse_taken(v.data(), n);
    }
    v.resize(n);
    return v;
  });
  m.def("sgd_fuse_taken_master", []() {
    std::vector<uintptr_t> v(256);
    int n = ddp_sgd_fuse_taken_master(v.data(), (int)v.size());
    if (n > (int)v.size()) {
      v.resize(n);
      n = ddp_sgd_fuse_taken_master(v.data(), n);
    }
    v.resize(n);
    return v;
  });
  m.def("conv_dense2x2_set", [](int on) { ddp_conv_dense2x2_set(on); });
  m.def("conv_dense2x2_ok", [](py::tuple g) {
    auto c = geom(g);
    return ddp_conv_dense2x2_ok(&c) != 0;
  });
  m.def("conv_pair_mode", [](int mode, int items) { ddp_conv_pair_mode(mode, items); },
        py::arg("mode"), py::arg("items") = 0);
  m.def("conv_pair_force", [](int sd, int sw, int tile) { ddp_conv_pair_force(sd, sw, tile); },
        py::arg("splits_dg"), py::arg("splits_wg"), py::arg("tile") = 0);
  // final = 1: no DGRAD of this layer follows (its finish may apply a registered SGD step)
  m.def("conv_wgrad", [](py::tuple g, uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws,
                         size_t ws_elems, int splits, uintptr_t st, int final_) {
    auto c = geom(g);
    if (final_)
      check(ddp_conv_wgrad_final(&c, P<void>(dy), P<void>(x), P<float>(dw), P<float>(ws),
                                 ws_elems, splits, S(st)), "conv_wgrad");
    else
      check(ddp_conv_wgrad(&c, P<void>(dy), P<void>(x), P<float>(dw), P<float>(ws), ws_elems,
                           splits, S(st)), "conv_wgrad");
  }, py::arg("g"), py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("ws"), py::arg("ws_elems"),
     py::arg("splits"), py::arg("stream"), py::arg("final") = 0);

  m.def("bn_act_fwd", [](int N, int H, int W, int C, int pool, int relu, float eps, uintptr_t z,
                         uintptr_t res, uintptr_t stats, uintptr_t gamma, uintptr_t beta,
                         uintptr_t out, uintptr_t st, uintptr_t running_mean,
                         uintptr_t running_var, float momentum, int use_running, uintptr_t coef,
                         uintptr_t mask, uintptr_t rstats, uintptr_t rgamma, uintptr_t rbeta,
                         uintptr_t rcoef, uintptr_t rrunning_mean, uintptr_t rrunning_var,
                         float reps, float rmomentum) {
    ddp_amd::BnArgs a{};
    a.coef = P<float>(coef);
    a.mask = P<unsigned char>(mask);
    a.N = N; a.H = H; a.W = W; a.C = C; a.pool = pool; a.relu = relu; a.eps = eps;
    a.z = P<unsigned short>(z); a.res = P<unsigned short>(res); a.stats = P<float>(stats);
    a.gamma = P<float>(gamma); a.beta = P<float>(beta); a.out = P<unsigned short>(out);
    a.running_mean = P<float>(running_mean); a.running_var = P<float>(running_var);
    a.momentum = momentum; a.use_running = use_running;
    if (rcoef) {  // res = the projection shortcut's pre-BN output, r = its BatchNorm
      ddp_amd::BnArgs r{};
      r.C = C; r.eps = reps; r.momentum = rmomentum;
      r.stats = P<float>(rstats); r.gamma = P<float>(rgamma); r.beta = P<float>(rbeta);
      r.coef = P<float>(rcoef);
      r.running_mean = P<float>(rrunning_mean); r.running_var = P<float>(rrunning_var);
      a.rcoef = r.coef;
      check(ddp_bn_act_fwd_res(&a, &r, S(st)), "bn_act_fwd (shortcut BN)");
      return;
    }
    check(ddp_bn_act_fwd(&a, S(st)), "bn_act_fwd");
  }, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("pool"), py::arg("relu"),
     py::arg("eps"), py::arg("z"), py::arg("res"), py::arg("stats"), py::arg("gamma"),
     py::arg("beta"), py::arg("out"), py::arg("stream"), py::arg("running_mean") = 0,
     py::arg("running_var") = 0, py::arg("momentum") = 0.1f, py::arg("use_running") = 0,
     py::arg("coef") = 0, py::arg("mask") = 0, py::arg("rstats") = 0, py::arg("rgamma") = 0,
     py::arg("rbeta") = 0, py::arg("rcoef") = 0, py::arg("rrunning_mean") = 0,
     py::arg("rrunning_var") = 0, py::arg("reps") = 1e-5f, py::arg("rmomentum") = 0.1f);
  m.def("maxpool_fwd", [](uintptr_t x, int N, int H, int W, int C, int KH, int KW, int stride,
                          int pad, int Ho, int Wo, uintptr_t y, uintptr_t idx, uintptr_t st) {
    check(ddp_maxpool_fwd(P<void>(x), N, H, W, C, KH, KW, stride, pad, Ho, Wo, P<void>(y),
                          P<void>(idx), S(st)), "maxpool_fwd");
  });
  m.def("maxpool_bwd", [](uintptr_t dy, uintptr_t idx, int N, int H, int W, int C, int KH, int KW,
                          int stride, int pad, int Ho, int Wo, uintptr_t dx, uintptr_t st) {
    check(ddp_maxpool_bwd(P<void>(dy), P<void>(idx), N, H, W, C, KH, KW, stride, pad, Ho, Wo,
                          P<void>(dx), S(st)), "maxpool_bwd");
  });
  m.def("avgpool_fwd", [](uintptr_t x, int N, int HW, int C, uintptr_t y, uintptr_t st) {
    check(ddp_avgpool_fwd(P<void>(x), N, HW, C, P<void>(y), S(st)), "avgpool_fwd");
  });
  m.def("avgpool_bwd", [](uintptr_t dy, int N, int HW, int C, uintptr_t dx, uintptr_t st) {
    check(ddp_avgpool_bwd(P<void>(dy), N, HW, C, P<void>(dx), S(st)), "avgpool_bwd");
  });
  m.def("colsum", [](uintptr_t dl, int B, int J, uintptr_t db, uintptr_t st) {
    check(ddp_colsum(P<void>(dl), B, J, P<float>(db), S(st)), "colsum");
  });
  m.def("bn_act_bwd", [](int N, int H, int W, int C, int pool, int relu, float eps, uintptr_t z,
                         uintptr_t res, uintptr_t stats, uintptr_t gamma, uintptr_t beta,
                         uintptr_t dout, uintptr_t sums, uintptr_t dz, uintptr_t dres,
                         uintptr_t dgamma, uintptr_t dbeta, uintptr_t dbias, uintptr_t st,
                         uintptr_t coef, int sums_ready, uintptr_t mask, uintptr_t rcoef,
                         uintptr_t rsums, uintptr_t rdz, uintptr_t rdgamma, uintptr_t rdbeta) {
    ddp_amd::BnArgs a{};
    a.coef = P<float>(coef);
    a.sums_ready = sums_ready;
    a.mask = P<unsigned char>(mask);
    a.N = N; a.H = H; a.W = W; a.C = C; a.pool = pool; a.relu = relu; a.eps = eps;
    a.z = P<unsigned short>(z); a.res = P<unsigned short>(res); a.stats = P<float>(stats);
    a.gamma = P<float>(gamma); a.beta = P<float>(beta); a.dout = P<unsigned short>(dout);
    a.sums = P<float>(sums); a.dz = P<unsigned short>(dz); a.dres = P<unsigned short>(dres);
    a.dgamma = P<float>(dgamma); a.dbeta = P<float>(dbeta); a.dbias = P<float>(dbias);
    if (rcoef) {  // res = the projection shortcut's pre-BN output: its dz goes to rdz
      a.rcoef = P<float>(rcoef); a.rsums = P<float>(rsums); a.rdz = P<unsigned short>(rdz);
      a.rdgamma = P<float>(rdgamma); a.rdbeta = P<float>(rdbeta);
      check(ddp_bn_act_bwd_res(&a, S(st)), "bn_act_bwd (shortcut BN)");
      return;
    }
    check(ddp_bn_act_bwd(&a, S(st)), "bn_act_bwd");
  }, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("pool"), py::arg("relu"),
     py::arg("eps"), py::arg("z"), py::arg("res"), py::arg("stats"), py::arg("gamma"),
     py::arg("beta"), py::arg("dout"), py::arg("sums"), py::arg("dz"), py::arg("dres"),
     py::arg("dgamma"), py::arg("dbeta"), py::arg("dbias"), py::arg("stream"), py::arg("coef"),
     py::arg("sums_ready") = 0, py::arg("mask") = 0, py::arg("rcoef") = 0, py::arg("rsums") = 0,
     py::arg("rdz") = 0, py::arg("rdgamma") = 0, py::arg("rdbeta") = 0);
  // ResNet stem: BN + ReLU + MaxPool2d(3, 2, 1) in one pass each way (bn_act.hip bn_pool3_*):
  // (N, H, W) = conv output, out / dout pooled, idx = uint8 window argmax (pooled shape)
  m.def("bn_pool3_fwd", [](int N, int H, int W, int C, int relu, float eps, uintptr_t z,
                           uintptr_t stats, uintptr_t gamma, uintptr_t beta, uintptr_t out,
                           uintptr_t idx, uintptr_t st, uintptr_t running_mean,
                           uintptr_t running_var, float momentum, int use_running, uintptr_t coef) {
    ddp_amd::BnArgs a{};
    a.N = N; a.H = H; a.W = W; a.C = C; a.relu = relu; a.eps = eps;
    a.z = P<unsigned short>(z); a.stats = P<float>(stats); a.gamma = P<float>(gamma);
    a.beta = P<float>(beta); a.out = P<unsigned short>(out); a.coef = P<float>(coef);
    a.running_mean = P<float>(running_mean); a.running_var = P<float>(running_var);
    a.momentum = momentum; a.use_running = use_running;
    check(ddp_bn_pool3_fwd(&a, P<unsigned char>(idx), S(st)), "bn_pool3_fwd");
  });
  m.def("bn_pool3_bwd", [](int N, int H, int W, int C, int relu, float eps, uintptr_t z,
                           uintptr_t dout, uintptr_t idx, uintptr_t sums, uintptr_t dz,
                           uintptr_t dgamma, uintptr_t dbeta, uintptr_t st, uintptr_t coef) {
    ddp_amd::BnArgs a{};
    a.N = N; a.H = H; a.W = W; a.C = C; a.relu = relu; a.eps = eps;
    a.z = P<unsigned short>(z); a.dout = P<unsigned short>(dout); a.sums = P<float>(sums);
    a.dz = P<unsigned short>(dz); a.dgamma = P<float>(dgamma); a.dbeta = P<float>(dbeta);
    a.coef = P<float>(coef);
    check(ddp_bn_pool3_bwd(&a, P<unsigned char>(idx), S(st)), "bn_pool3_bwd");
  });
  m.def("bn_bwd_local_ok", [](int N, int H, int W, int C, int pool) {
    return ddp_bn_bwd_local_ok(N, H, W, C, pool) != 0;
  });
  m.def("bn_bwd_local_set", [](long long max_loads) { ddp_bn_bwd_local_set(max_loads); });
  m.def("conv_epi_stage_set", [](int on) { ddp_conv_epi_stage_set(on); });

  // ``soft`` (here and in the two loss entry points below): None = the plain kernel, else
  // (smoothing, partner-label pointer | 0, lam pointer | 0) = api.h SoftTarget
  m.def("linear_ce_fwd", [](uintptr_t x, uintptr_t W, uintptr_t b, uintptr_t labels, int B, int F,
                            int J, uintptr_t logits, uintptr_t dlogits, uintptr_t loss_sum,
                            uintptr_t correct, uintptr_t st, uintptr_t loss_acc, py::object soft) {
    if (!soft.is_none()) {
      const ddp_amd::SoftTarget s = soft_target(soft);
      check(ddp_linear_ce_fwd_soft(nullptr, P<void>(x), P<float>(W), P<float>(b),
                                   P<long long>(labels), B, F, J, P<float>(logits),
                                   P<float>(dlogits), P<float>(loss_sum), P<int>(correct),
                                   P<float>(loss_acc), &s, S(st)), "linear_ce_fwd (soft)");
      return;
    }
    check(ddp_linear_ce_fwd(P<void>(x), P<float>(W), P<float>(b), P<long long>(labels), B, F, J,
                            P<float>(logits), P<float>(dlogits), P<float>(loss_sum),
                            P<int>(correct), P<float>(loss_acc), S(st)), "linear_ce_fwd");
  }, py::arg("x"), py::arg("W"), py::arg("b"), py::arg("labels"), py::arg("B"), py::arg("F"),
     py::arg("J"), py::arg("logits"), py::arg("dlogits"), py::arg("loss_sum"), py::arg("correct"),
     py::arg("stream"), py::arg("loss_acc") = 0, py::arg("soft") = py::none());
  // the head with the last block's BN + ReLU + 2x2 pool folded in (writes the features y)
  m.def("bn_pool_linear_ce_fwd", [](uintptr_t z, uintptr_t stats, uintptr_t gamma, uintptr_t beta,
                                    float eps, int relu, uintptr_t coef, uintptr_t y, uintptr_t W,
                                    uintptr_t b, uintptr_t labels, int B, int F, int J,
                                    uintptr_t dlogits, uintptr_t loss_sum, uintptr_t st,
                                    uintptr_t loss_acc, py::object soft) {
    ddp_amd::HeadBnIn h{P<unsigned short>(z), P<float>(stats), P<float>(gamma), P<float>(beta),
                        eps, relu, P<float>(coef), P<unsigned short>(y)};
    if (!soft.is_none()) {
      const ddp_amd::SoftTarget s = soft_target(soft);
      check(ddp_linear_ce_fwd_soft(&h, nullptr, P<float>(W), P<float>(b), P<long long>(labels), B,
                                   F, J, nullptr, P<float>(dlogits), P<float>(loss_sum), nullptr,
                                   P<float>(loss_acc), &s, S(st)), "bn_pool_linear_ce_fwd (soft)");
      return;
    }
    check(ddp_bn_pool_linear_ce_fwd(&h, P<float>(W), P<float>(b), P<long long>(labels), B, F, J,
                                    P<float>(dlogits), P<float>(loss_sum), nullptr,
                                    P<float>(loss_acc), S(st)), "bn_pool_linear_ce_fwd");
  }, py::arg("z"), py::arg("stats"), py::arg("gamma"), py::arg("beta"), py::arg("eps"),
     py::arg("relu"), py::arg("coef"), py::arg("y"), py::arg("W"), py::arg("b"), py::arg("labels"),
     py::arg("B"), py::arg("F"), py::arg("J"), py::arg("dlogits"), py::arg("loss_sum"),
     py::arg("stream"), py::arg("loss_acc") = 0, py::arg("soft") = py::none());
  m.def("linear_bwd", [](uintptr_t dlogits, uintptr_t x, uintptr_t W, int B, int F, int J,
                         uintptr_t gscale, uintptr_t dx, uintptr_t dW, uintptr_t db,
                         uintptr_t st) {
    check(ddp_linear_bwd(P<float>(dlogits), P<void>(x), P<float>(W), B, F, J, P<float>(gscale),
                         P<void>(dx), P<float>(dW), P<float>(db), S(st)), "linear_bwd");
  });
  m.def("softmax_ce", [](uintptr_t logits, int bf16, uintptr_t labels, int B, int J,
                         uintptr_t loss_sum, uintptr_t correct, uintptr_t dlogits,
                         int dlogits_bf16, uintptr_t st, py::object soft) {
    if (!soft.is_none()) {
      const ddp_amd::SoftTarget s = soft_target(soft);
      check(ddp_softmax_ce_soft(P<void>(logits), bf16, P<long long>(labels), B, J,
                                P<float>(loss_sum), P<int>(correct), P<void>(dlogits),
                                dlogits_bf16, &s, S(st)), "softmax_ce (soft)");
      return;
    }
    check(ddp_softmax_ce(P<void>(logits), bf16, P<long long>(labels), B, J, P<float>(loss_sum),
                         P<int>(correct), P<void>(dlogits), dlogits_bf16, S(st)), "softmax_ce");
  }, py::arg("logits"), py::arg("bf16"), py::arg("labels"), py::arg("B"), py::arg("J"),
     py::arg("loss_sum"), py::arg("correct"), py::arg("dlogits"), py::arg("dlogits_bf16"),
     py::arg("stream"), py::arg("soft") = py::none());

  m.def("sgd", [](uintptr_t p, uintptr_t g, uintptr_t buf, size_t n, float lr, float momentum,
                  float wd, float grad_scale, int nesterov, uintptr_t st, uintptr_t sched) {
    check(ddp_sgd(P<float>(p), P<float>(g), P<float>(buf), n, lr, momentum, wd, grad_scale,
                  nesterov, P<const ddp_amd::LrSched>(sched), S(st)), "sgd");
  }, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("n"), py::arg("lr"), py::arg("momentum"),
     py::arg("wd"), py::arg("grad_scale"), py::arg("nesterov"), py::arg("stream"),
     py::arg("sched") = 0);
  m.def("conv_options", [](int stages) { ddp_conv_options(stages); }, py::arg("stages") = 2);
  // measured tile/split table (mode 0 fwd, 1 dgrad, 2 wgrad; GEMM dims M, N, K; tile 0..3 =
  // 128x128, 128x64, 64x128, 64x64) and the forced-tile switch used by tools/conv_tune.py
  m.def("conv_tune_set", [](int mode, int M, int N, int K, int tile, int splits, int stages) {
    ddp_conv_tune_set(mode, M, N, K, tile, splits, stages);
  }, py::arg("mode"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("tile"),
     py::arg("splits"), py::arg("stages") = 0);
  m.def("conv_tune_clear", []() { ddp_conv_tune_clear(); });
  m.def("conv_wgrad_pm_set", [](int on) { ddp_conv_wgrad_pm_set(on); });
  m.def("conv_rows_pm_set", [](int on) { ddp_conv_rows_pm_set(on); });
  m.def("bn_fold_bwd_mb", [](int mb) { ddp_bn_fold_bwd_mb(mb); });
  m.def("bn_fold_grid", [](int blocks) { ddp_bn_fold_grid(blocks); });
  m.def("conv_pair_tune_set", [](int M, int N, int K, int hw, int tile, int sd, int sw) {
    ddp_conv_pair_tune_set(M, N, K, hw, tile, sd, sw);
  });
  m.def("conv_force_tile", [](int t, int stages) { ddp_conv_force_tile(t, stages); },
        py::arg("tile_plus_one"), py::arg("stages") = 0);
#ifdef DDP_CONV_STAMPS
  m.def("conv_stamps_set", [](uintptr_t buf, int cap) { ddp_conv_stamps_set(P<void>(buf), cap); });
#endif
  m.def("pack_conv_weights", [](const std::vector<PackTuple>& descs, uintptr_t st) {
    auto d = pack_descs(descs);
    check(ddp_pack_conv_weights(d.data(), (int)d.size(), S(st)), "pack_conv_weights");
  });
  m.def("sgd_pack", [](uintptr_t items, int n_items, uintptr_t descs, uintptr_t p, uintptr_t g,
                       uintptr_t buf, float lr, float momentum, float wd, float grad_scale,
                       int nesterov, uintptr_t st, int zero_grad, uintptr_t counter, int delta,
                       uintptr_t skip, uintptr_t shadow, uintptr_t slot, uintptr_t done,
                       uintptr_t signal, uintptr_t sched, int sched_advance, uintptr_t lars_side,
                       uintptr_t lars_tensors, uintptr_t lars_partial, uintptr_t lars_trust,
                       float lars_eta, float lars_eps, uintptr_t clip_partial, int clip_chunks,
                       float clip_max_norm, float clip_eps, int clip_flags,
                       uintptr_t clip_stats, uintptr_t ema, float ema_one_minus_decay,
                       uintptr_t adam_v, uintptr_t adam_bias, unsigned adam_n_bias,
                       float adam_omb1, float adam_beta2, float adam_omb2, float adam_eps,
                       uintptr_t lamb_side, uintptr_t lamb_tensors, uintptr_t lamb_partial,
                       uintptr_t lamb_trust) {
    ddp_amd::UpdateLaunch u{};
    u.items = P<int4>(items); u.descs = P<ddp_amd::ConvDesc>(descs);
    u.p = P<float>(p); u.g = P<float>(g); u.buf = P<float>(buf);
    u.h = {lr, momentum, wd, grad_scale, nesterov, zero_grad, P<int>(counter), delta,
           P<const unsigned>(skip), P<unsigned short>(shadow), P<float>(slot), P<unsigned>(done),
           P<unsigned>(signal), P<ddp_amd::LrSched>(sched), sched_advance};
    u.n_items = n_items;
    u.lars = {P<int2>(lars_side), P<int4>(lars_tensors), P<float2>(lars_partial),
              P<float>(lars_trust), lars_eta, lars_eps};
    u.clip = {P<const float>(clip_partial), clip_chunks, clip_max_norm, clip_eps, clip_flags,
              P<float>(clip_stats)};
    u.ema = {P<float>(ema), ema_one_minus_decay};
    u.adam = {P<float>(adam_v), P<const float2>(adam_bias), adam_n_bias, adam_omb1, adam_beta2,
              adam_omb2, adam_eps};
    u.lamb = {P<int2>(lamb_side), P<int4>(lamb_tensors), P<float2>(lamb_partial),
              P<float>(lamb_trust)};
    check(ddp_sgd_pack(&u, S(st)), "sgd_pack");
  }, py::arg("items"), py::arg("n_items"), py::arg("descs"), py::arg("p"), py::arg("g"),
     py::arg("buf"), py::arg("lr"), py::arg("momentum"), py::arg("wd"), py::arg("grad_scale"),
     py::arg("nesterov"), py::arg("stream"), py::arg("zero_grad") = 0, py::arg("counter") = 0,
     py::arg("delta") = 0, py::arg("skip") = 0, py::arg("shadow") = 0, py::arg("slot") = 0,
     py::arg("done") = 0, py::arg("signal") = 0, py::arg("sched") = 0,
     py::arg("sched_advance") = 0, py::arg("lars_side") = 0, py::arg("lars_tensors") = 0,
     py::arg("lars_partial") = 0, py::arg("lars_trust") = 0, py::arg("lars_eta") = 0.f,
     py::arg("lars_eps") = 0.f, py::arg("clip_partial") = 0, py::arg("clip_chunks") = 0,
     py::arg("clip_max_norm") = 0.f, py::arg("clip_eps") = 0.f, py::arg("clip_flags") = 0,
     py::arg("clip_stats") = 0, py::arg("ema") = 0, py::arg("ema_one_minus_decay") = 0.f,
     py::arg("adam_v") = 0, py::arg("adam_bias") = 0, py::arg("adam_n_bias") = 0,
     py::arg("adam_omb1") = 0.f, py::arg("adam_beta2") = 0.f, py::arg("adam_omb2") = 0.f,
     py::arg("adam_eps") = 0.f, py::arg("lamb_side") = 0, py::arg("lamb_tensors") = 0,
     py::arg("lamb_partial") = 0, py::arg("lamb_trust") = 0);
  // gradient guard (optim.hip chunk_sums_kernel<false>): per-chunk sum (g * grad_scale)^2 of every
  // parameter chunk in the items, the input of sgd_pack's clip_* arguments
  m.def("grad_sumsq", [](uintptr_t items, int n_items, uintptr_t g, float grad_scale,
                         uintptr_t partial, uintptr_t st) {
    check(ddp_grad_sumsq(P<void>(items), n_items, P<float>(g), grad_scale, P<float>(partial),
                         S(st)), "grad_sumsq");
  }, py::arg("items"), py::arg("n_items"), py::arg("grad"), py::arg("grad_scale"),
     py::arg("partial"), py::arg("stream"));
  // LARS norms launch (optim.hip chunk_sums_kernel<true>): per-chunk {sum p^2,
  // sum (g * grad_scale)^2}
  m.def("lars_norms", [](uintptr_t items, int n_items, uintptr_t p, uintptr_t g, float grad_scale,
                         uintptr_t partial, uintptr_t st) {
    check(ddp_lars_norms(P<void>(items), n_items, P<float>(p), P<float>(g), grad_scale,
                         P<void>(partial), S(st)), "lars_norms");
  }, py::arg("items"), py::arg("n_items"), py::arg("p"), py::arg("g"), py::arg("grad_scale"),
     py::arg("partial"), py::arg("stream"));
  // LAMB norms launch (optim.hip lamb_norms_kernel): per-chunk {sum p^2, sum r^2}, r the update
  // direction of api.h LambArgs; adam_* as sgd_pack's, clip_* select the guarded instantiation
  m.def("lamb_norms", [](uintptr_t items, int n_items, uintptr_t p, uintptr_t g, uintptr_t m,
                         float wd, float grad_scale, uintptr_t partial, uintptr_t st,
                         uintptr_t sched, uintptr_t adam_v, uintptr_t adam_bias,
                         unsigned adam_n_bias, float adam_omb1, float adam_beta2, float adam_omb2,
                         float adam_eps, uintptr_t clip_partial, int clip_chunks,
                         float clip_max_norm, float clip_eps, int clip_flags) {
    ddp_amd::LambNorms n{};
    n.items = P<int4>(items); n.n_items = n_items;
    n.p = P<float>(p); n.g = P<float>(g); n.m = P<float>(m);
    n.sched = P<ddp_amd::LrSched>(sched); n.wd = wd; n.grad_scale = grad_scale;
    n.adam = {P<float>(adam_v), P<const float2>(adam_bias), adam_n_bias, adam_omb1, adam_beta2,
              adam_omb2, adam_eps};
    n.partial = P<float2>(partial);
    n.clip = {P<const float>(clip_partial), clip_chunks, clip_max_norm, clip_eps, clip_flags,
              nullptr};
    check(ddp_lamb_norms(&n, S(st)), "lamb_norms");
  }, py::arg("items"), py::arg("n_items"), py::arg("p"), py::arg("g"), py::arg("m"),
     py::arg("wd"), py::arg("grad_scale"), py::arg("partial"), py::arg("stream"),
     py::arg("sched") = 0, py::arg("adam_v") = 0, py::arg("adam_bias") = 0,
     py::arg("adam_n_bias") = 0, py::arg("adam_omb1") = 0.f, py::arg("adam_beta2") = 0.f,
     py::arg("adam_omb2") = 0.f, py::arg("adam_eps") = 0.f, py::arg("clip_partial") = 0,
     py::arg("clip_chunks") = 0, py::arg("clip_max_norm") = 0.f, py::arg("clip_eps") = 0.f,
     py::arg("clip_flags") = 0);
  m.def("shard_tail", [](uintptr_t segs, int n_segs, uintptr_t src, uintptr_t dst,
                         const std::vector<PackTuple>& descs, uintptr_t done, uintptr_t signal,
                         uintptr_t skip, uintptr_t st) {
    auto d = pack_descs(descs);
    check(ddp_shard_tail(P<void>(segs), n_segs, P<float>(src), P<float>(dst), d.data(),
                         (int)d.size(), P<unsigned>(done), P<unsigned>(signal),
                         P<const unsigned>(skip), S(st)), "shard_tail");
  });
  m.def("seg_copy_f32", [](uintptr_t table, int n, uintptr_t src, uintptr_t dst, uintptr_t st) {
    check(ddp_seg_copy_f32(P<void>(table), n, P<float>(src), P<float>(dst), S(st)), "seg_copy_f32");
  });
  m.def("sgd_tile_dims", [](int RS) {
    int tk, tc;
    ddp_sgd_tile_dims(RS, &tk, &tc);
    return std::make_pair(tk, tc);
  });
  m.def("sgd_tile_limit", []() { return ddp_sgd_tile_limit(); });
  // sched (api.h LrSched) with sched_mode 1: whole advance, 2: the staged step becomes current
  m.def("counter_add", [](uintptr_t c, int delta, uintptr_t st, uintptr_t sched, int sched_mode) {
    check(ddp_counter_add(P<int>(c), delta, P<ddp_amd::LrSched>(sched), sched_mode, S(st)),
          "counter_add");
  }, py::arg("c"), py::arg("delta"), py::arg("stream"), py::arg("sched") = 0,
     py::arg("sched_mode") = 0);

  m.def("synth_generate", [](uintptr_t images, uintptr_t labels, int n, int pix_per_img,
                             unsigned int seed, int classes, uintptr_t st) {
    check(ddp_synth_generate(P<unsigned char>(images), P<int>(labels), n, pix_per_img, seed,
                             classes, S(st)), "synth_generate");
  });
  m.def("augment", [](uintptr_t images, uintptr_t labels, uintptr_t indices, uintptr_t cursor,
                      int L, int B, int H, int W, int Cp, int pad, int flip, unsigned int seed,
                      unsigned int epoch, std::vector<float> mean, std::vector<float> std_,
                      uintptr_t x, uintptr_t y, uintptr_t st, uintptr_t zero, size_t zero_n,
                      uintptr_t sched, int cursor_off, py::object mix) {
    ddp_amd::AugArgs a{};
    a.cursor_off = cursor_off;
    a.sched = P<ddp_amd::LrSched>(sched);
    a.zero = P<float>(zero);
    a.zero_n = zero ? zero_n : 0;
    a.images = P<unsigned char>(images); a.labels = P<int>(labels); a.indices = P<int>(indices);
    a.cursor = P<int>(cursor); a.L = L; a.B = B; a.H = H; a.W = W; a.Cp = Cp; a.pad = pad;
    a.flip = flip; a.seed = seed; a.epoch = epoch;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean.at(c); a.inv_std[c] = 1.f / std_.at(c); }
    a.x = P<unsigned short>(x); a.y = P<long long>(y);
    if (!mix.is_none()) {  // mixup: (y2, lam table, entries, lam_cur) = api.h MixArgs
      auto t = mix.cast<py::tuple>();
      if (t.size() != 4) throw std::runtime_error("mix needs (y2, table, n, lam_cur)");
      const ddp_amd::MixArgs mx{P<long long>(t[0].cast<uintptr_t>()),
                                P<float>(t[1].cast<uintptr_t>()), t[2].cast<int>(),
                                P<float>(t[3].cast<uintptr_t>())};
      check(ddp_augment_mix(&a, &mx, S(st)), "augment (mixup)");
      return;
    }
    check(ddp_augment(&a, S(st)), "augment");
  }, py::arg("images"), py::arg("labels"), py::arg("indices"), py::arg("cursor"), py::arg("L"),
     py::arg("B"), py::arg("H"), py::arg("W"), py::arg("Cp"), py::arg("pad"), py::arg("flip"),
     py::arg("seed"), py::arg("epoch"), py::arg("mean"), py::arg("std"), py::arg("x"),
     py::arg("y"), py::arg("stream"), py::arg("zero") = 0, py::arg("zero_n") = 0,
     py::arg("sched") = 0, py::arg("cursor_off") = 0, py::arg("mix") = py::none());
  m.def("nchw_to_nhwc", [](uintptr_t x, int N, int C, int H, int W, int Cp, uintptr_t out,
                           uintptr_t st) {
    check(ddp_nchw_to_nhwc(P<float>(x), N, C, H, W, Cp, P<void>(out), S(st)), "nchw_to_nhwc");
  });
  m.def("mean_ws", [](uintptr_t in, size_t n, int ws, uintptr_t out, uintptr_t st) {
    check(ddp_mean_ws(P<float>(in), n, ws, P<float>(out), S(st)), "mean_ws");
  });
  m.def("comm_standin", [](uintptr_t x, size_t n, int blocks, float usec, float scale, uintptr_t st,
                           int passes) {
    check(ddp_comm_standin(P<float>(x), n, blocks, usec, scale, passes, S(st)), "comm_standin");
  }, py::arg("x"), py::arg("n"), py::arg("blocks"), py::arg("usec"), py::arg("scale"),
     py::arg("stream"), py::arg("passes") = 1);
  m.def("flag_signal", [](uintptr_t flag, uintptr_t st) {
    check(ddp_flag_signal(P<unsigned>(flag), S(st)), "flag_signal");
  });
  m.def("flag_wait", [](uintptr_t flag, uintptr_t expected, uintptr_t err, float timeout_s,
                        uintptr_t st) {
    check(ddp_flag_wait(P<unsigned>(flag), P<unsigned>(expected), P<unsigned>(err), timeout_s,
                        S(st)),
          "flag_wait");
  });
  m.def("pack_bf16", [](uintptr_t x, size_t n, uintptr_t y, uintptr_t st) {
    check(ddp_pack_bf16(P<float>(x), n, P<unsigned short>(y), S(st)), "pack_bf16");
  });
  m.def("unpack_bf16", [](uintptr_t y, size_t n, uintptr_t x, uintptr_t st) {
    check(ddp_unpack_bf16(P<unsigned short>(y), n, P<float>(x), S(st)), "unpack_bf16");
  });
  // raw hipMemsetAsync / hipMemcpyAsync (D2D): tests/test_gpu_graph_memset.py checks the
  // ordering of captured memset / memcpy graph nodes against kernel nodes (the library itself
  // uses the copy / fill kernels above inside captured steps)
  m.def("memset_async", [](uintptr_t p, int value, size_t n, uintptr_t st) {
    check((int)hipMemsetAsync(P<void>(p), value, n, S(st)), "hipMemsetAsync");
  });
  m.def("memcpy_async", [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t st) {
    check((int)hipMemcpyAsync(P<void>(dst), P<void>(src), n, hipMemcpyDeviceToDevice, S(st)),
          "hipMemcpyAsync");
  });
  m.def("copy_bytes", [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t st) {
    check(ddp_copy_bytes(P<void>(dst), P<void>(src), n, S(st)), "copy_bytes");
  });
  m.def("fill_bytes", [](uintptr_t dst, int value, size_t n, uintptr_t st) {
    check(ddp_fill_bytes(P<void>(dst), value, n, S(st)), "fill_bytes");
  });
  m.def("scale", [](uintptr_t x, size_t n, float s, uintptr_t st) {
    check(ddp_scale(P<float>(x), n, s, S(st)), "scale");
  });

  // ---------------- communication runtime ----------------
  m.def("plan_buckets", [](std::vector<size_t> offsets, std::vector<size_t> numels,
                           size_t elem_bytes, size_t cap, size_t cap_first) {
    auto b = ddp_amd::plan_buckets(offsets, numels, elem_bytes, cap, cap_first);
    std::vector<std::tuple<int, int, size_t, size_t>> out;
    for (auto& x : b) out.emplace_back(x.first_param, x.last_param, x.offset, x.count);
    return out;
  });
  m.def("make_unique_id", []() { return py::bytes(RcclComm::make_unique_id()); });
  // BatchNorm statistics replicas per accumulator (api.h kStatRep) and whether this is the
  // deterministic-statistics build (_build.py variant "det")
  m.def("stat_replicas", []() { return ddp_amd::kStatRep; });
  m.def("deterministic", []() { return ddp_amd::kDeterministic; });

  // host-only readiness / launch-order state machine (no GPU needed: CPU tests drive it with
  // the same hook orders as the Python twin, tests/test_bucket_scheduler_cpu.py)
  py::class_<ddp_amd::BucketScheduler>(m, "BucketScheduler")
      .def(py::init([](std::vector<std::tuple<int, int, size_t, size_t>> bs, int n_params) {
             std::vector<ddp_amd::BucketSpec> v;
             for (auto& t : bs)
               v.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)});
             return new ddp_amd::BucketScheduler(v, n_params);
           }))
      .def("mark", &ddp_amd::BucketScheduler::mark)
      .def("finish", &ddp_amd::BucketScheduler::finish)
      .def("prepare", &ddp_amd::BucketScheduler::prepare)
      .def("launched", &ddp_amd::BucketScheduler::launched)
      .def("launch_order", &ddp_amd::BucketScheduler::launch_order)
      .def("set_launch_order", &ddp_amd::BucketScheduler::set_launch_order)
      .def("order_from_ready", &ddp_amd::BucketScheduler::order_from_ready)
      .def("ready_order", &ddp_amd::BucketScheduler::ready_order)
      .def("launch_log", &ddp_amd::BucketScheduler::launch_log);

  py::class_<StreamLink>(m, "StreamLink")
      .def(py::init<>())
      .def("link", &StreamLink::link)
      .def("record", &StreamLink::record)
      .def("wait", &StreamLink::wait);
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init([](int rank, int world, std::string uid, int device) {
             // ncclCommInitRank blocks until every rank joins: release the GIL meanwhile
             py::gil_scoped_release nogil;
             return new RcclComm(rank, world, uid, device);
           }),
           py::arg("rank"), py::arg("world"), py::arg("uid"), py::arg("device"))
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("world", &RcclComm::world)
      .def_property_readonly("live", &RcclComm::live)
      .def("count", &RcclComm::count)
      .def_static("version", &RcclComm::version)
      .def("all_reduce", [](RcclComm& c, uintptr_t buf, size_t n, int dt, int op, uintptr_t st) {
        c.all_reduce(P<void>(buf), n, dt, op, S(st));
      })
      .def("broadcast", [](RcclComm& c, uintptr_t buf, size_t n, int dt, int root, uintptr_t st) {
        c.broadcast(P<void>(buf), n, dt, root, S(st));
      })
      .def("all_gather", [](RcclComm& c, uintptr_t s, uintptr_t r, size_t n, int dt, uintptr_t st) {
        c.all_gather(P<void>(s), P<void>(r), n, dt, S(st));
      })
      .def("all_gather2", [](RcclComm& c, uintptr_t s1, uintptr_t r1, size_t n1, int dt1,
                             uintptr_t s2, uintptr_t r2, size_t n2, int dt2, uintptr_t st) {
        c.all_gather2(P<void>(s1), P<void>(r1), n1, dt1, P<void>(s2), P<void>(r2), n2, dt2, S(st));
      })
      .def("reduce_scatter", [](RcclComm& c, uintptr_t s, uintptr_t r, size_t n, int dt, int op,
                                uintptr_t st) { c.reduce_scatter(P<void>(s), P<void>(r), n, dt, op, S(st)); })
      .def("gather", [](RcclComm& c, uintptr_t s, uintptr_t r, size_t n, int dt, int root,
                        uintptr_t st) { c.gather(P<void>(s), P<void>(r), n, dt, root, S(st)); })
      .def("scatter", [](RcclComm& c, uintptr_t s, uintptr_t r, size_t n, int dt, int root,
                         uintptr_t st) { c.scatter(P<void>(s), P<void>(r), n, dt, root, S(st)); })
      .def("scatter_replicated", [](RcclComm& c, uintptr_t b, size_t n, int dt, int root,
                                    uintptr_t st) { c.scatter_replicated(P<void>(b), n, dt, root, S(st)); })
      .def("send", [](RcclComm& c, uintptr_t b, size_t n, int dt, int peer, uintptr_t st) {
        c.send(P<void>(b), n, dt, peer, S(st));
      })
      .def("recv", [](RcclComm& c, uintptr_t b, size_t n, int dt, int peer, uintptr_t st) {
        c.recv(P<void>(b), n, dt, peer, S(st));
      })
      .def("reserve_stage", &RcclComm::reserve_stage)
      .def("async_error", &RcclComm::async_error)
      .def("abort", &RcclComm::abort);

  py::class_<Reducer>(m, "Reducer")
      .def(py::init([](RcclComm* comm, uintptr_t arena, std::vector<size_t> offsets,
                       std::vector<size_t> numels, size_t cap, size_t cap_first, bool avg) {
             return new Reducer(comm, P<float>(arena), offsets, numels, cap, cap_first, avg);
           }),
           py::keep_alive<1, 2>())
      .def("buckets", [](Reducer& r) {
        std::vector<std::tuple<int, int, size_t, size_t>> out;
        for (auto& x : r.buckets()) out.emplace_back(x.first_param, x.last_param, x.offset, x.count);
        return out;
      })
      .def("prepare", &Reducer::prepare)
      .def("mark_ready", [](Reducer& r, int p, uintptr_t st) { r.mark_ready(p, S(st)); })
      .def("finalize", [](Reducer& r, uintptr_t st) { r.finalize(S(st)); })
      .def("set_debug_sync", &Reducer::set_debug_sync)
      .def("set_overlap", &Reducer::set_overlap)
      .def("overlap", &Reducer::overlap)
      .def("set_emulate", &Reducer::set_emulate)
      .def("set_emulate_passes", &Reducer::set_emulate_passes)
      .def("set_emulate_bw", &Reducer::set_emulate_bw, py::arg("gbps"), py::arg("blocks") = 32)
      .def("set_comm_dtype", &Reducer::set_comm_dtype)
      .def("comm_dtype", &Reducer::comm_dtype)
      .def("launched", &Reducer::launched)
      .def("launch_order", [](Reducer& r) { return r.scheduler().launch_order(); })
      .def("set_launch_order", [](Reducer& r, std::vector<int> o) { r.scheduler().set_launch_order(o); })
      .def("order_from_ready", [](Reducer& r, std::vector<int> seq) { return r.scheduler().order_from_ready(seq); })
      .def("ready_order", [](Reducer& r) { return r.scheduler().ready_order(); })
      .def("launch_log", [](Reducer& r) { return r.scheduler().launch_log(); })
      .def("set_timing", &Reducer::set_timing)
      .def("bucket_times", [](Reducer& r, uintptr_t ref) {
        return r.bucket_times(reinterpret_cast<hipEvent_t>(ref));
      })
      .def("comm_stream", [](Reducer& r) { return reinterpret_cast<uintptr_t>(r.comm_stream()); });
}
