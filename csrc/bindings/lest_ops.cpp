// torch.ops.svoc.lest_round / lest_route: the rank-weighted (L-estimator) fast round.  CPU: the twin in
// reference_cpu.cpp (lest_round_batch_cpu); CUDA (= HIP): csrc/kernels/consensus_fast_lest.hip.  Out semantics, and
// shape / dtype / device checks only -- nothing is read back from the device, so a round can be graph-captured.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <thread>

#include "../engine/engine.hpp"
#include "svoc/route.hpp"

namespace svoc {
namespace {

int lest_cpu_threads() {
  static int n = [] {
    unsigned h = std::thread::hardware_concurrency();
    return (int)(h == 0 ? 1 : (h > 32 ? 32 : h));
  }();
  return n;
}

void lest_out(const at::Tensor& t, at::ScalarType dt, std::initializer_list<int64_t> shape, const char* name,
              const at::Device& dev) {
  TORCH_CHECK(t.scalar_type() == dt, name, ": wrong dtype ", t.scalar_type());
  TORCH_CHECK(t.device() == dev, name, ": wrong device");
  TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
  TORCH_CHECK(t.sizes().vec() == std::vector<int64_t>(shape), name, ": wrong shape ", t.sizes());
}

const uint8_t* lest_active(const c10::optional<at::Tensor>& active, int64_t B, const at::Device& dev) {
  if (!active.has_value() || !active->defined()) return nullptr;
  const auto& a = *active;
  TORCH_CHECK(a.scalar_type() == at::kByte || a.scalar_type() == at::kBool, "active: uint8/bool");
  TORCH_CHECK(a.numel() == B && a.is_contiguous() && a.device() == dev, "active: [B] contiguous");
  return (const uint8_t*)a.data_ptr();
}

void lest_checks(const at::Tensor& values, int64_t D, int64_t n_failing, const at::Tensor& weights, const at::Tensor& c1,
                 const at::Tensor& cons, const at::Tensor& skew, const at::Tensor& kurt, const at::Tensor& rel,
                 const at::Tensor& qr, const at::Tensor& reliable, const at::Tensor& status) {
  TORCH_CHECK(values.dim() == 3 && values.scalar_type() == at::kFloat, "lest_round: values fp32 [B, N, ld]");
  TORCH_CHECK(values.stride(2) == 1 && values.stride(1) == values.size(2), "values: rows must be dense");
  const int64_t B = values.size(0), N = values.size(1);
  TORCH_CHECK(D >= 1 && D <= values.size(2), "D must be <= ld");
  TORCH_CHECK(N >= 2, "lest_round: N >= 2");
  TORCH_CHECK(n_failing >= 0, "lest_round: n_failing >= 0");
  const auto dev = values.device();
  lest_out(weights, at::kFloat, {2, kLestWeightPitch}, "weights", dev);
  lest_out(c1, at::kFloat, {B, D}, "c1", dev);
  lest_out(cons, at::kFloat, {B, D}, "consensus", dev);
  lest_out(skew, at::kFloat, {B, D}, "skew", dev);
  lest_out(kurt, at::kFloat, {B, D}, "kurt", dev);
  lest_out(rel, at::kFloat, {B, 2}, "rel", dev);
  lest_out(qr, at::kFloat, {B, N}, "qr", dev);
  lest_out(reliable, at::kByte, {B, N}, "reliable", dev);
  lest_out(status, at::kInt, {B}, "status", dev);
}

void lest_round_cpu(const at::Tensor& values, const c10::optional<at::Tensor>& active, int64_t D, int64_t n_failing,
                    bool constrained, double max_spread, const at::Tensor& weights, at::Tensor c1, at::Tensor cons,
                    at::Tensor skew, at::Tensor kurt, at::Tensor rel, at::Tensor qr, at::Tensor reliable,
                    at::Tensor status, const c10::optional<at::Tensor>& work) {
  (void)work;   // (the GPU kernel's staging area)
  lest_checks(values, D, n_failing, weights, c1, cons, skew, kurt, rel, qr, reliable, status);
  const int64_t B = values.size(0), N = values.size(1), ld = values.size(2), is = values.stride(0);
  TORCH_CHECK(N <= kLestWeightPitch, "lest_round: N <= ", kLestWeightPitch, " (one weight per rank)");
  FastBatch fb;
  fb.values = values.data_ptr();
  fb.load = [=](const void* base, int64_t i, float* dst) {
    for (int64_t r = 0; r < N; ++r)
      for (int64_t d = 0; d < D; ++d) dst[r * D + d] = ((const float*)base)[i * is + r * ld + d];
  };
  fb.active = lest_active(active, B, values.device());
  fb.B = B; fb.N = N; fb.D = D;
  fb.n_failing = n_failing;
  fb.constrained = constrained;
  fb.max_spread = (float)max_spread;
  fb.c1 = c1.data_ptr<float>();
  fb.consensus = cons.data_ptr<float>();
  fb.rel = rel.data_ptr<float>();
  fb.skew = skew.data_ptr<float>();
  fb.kurt = kurt.data_ptr<float>();
  fb.reliable = reliable.data_ptr<uint8_t>();
  fb.qr = qr.data_ptr<float>();
  fb.status = status.data_ptr<int32_t>();
  lest_round_batch_cpu(fb, weights.data_ptr<float>(), lest_cpu_threads());
}

void lest_round_hip(const at::Tensor& values, const c10::optional<at::Tensor>& active, int64_t D, int64_t n_failing,
                    bool constrained, double max_spread, const at::Tensor& weights, at::Tensor c1, at::Tensor cons,
                    at::Tensor skew, at::Tensor kurt, at::Tensor rel, at::Tensor qr, at::Tensor reliable,
                    at::Tensor status, const c10::optional<at::Tensor>& work) {
  lest_checks(values, D, n_failing, weights, c1, cons, skew, kurt, rel, qr, reliable, status);
  const int64_t B = values.size(0), N = values.size(1), ld = values.size(2);
  TORCH_CHECK(B < (1ll << 31) && N < (1ll << 31) && ld < (1ll << 31) && D < (1 << 30) && n_failing < (1ll << 31),
              "size limits");
  // what the kernel takes (route.hpp lest_route), the same function its dispatcher switches on
  const LestRoute route = lest_route({kStoreF32, (int)N, (int)D, (int)ld, (int)n_failing, constrained, 0, 0, 0, kWorkCaller});
  TORCH_CHECK(route.supported, "lest_round: the GPU kernel takes fp32 storage, 2 <= N <= ", route.max_n,
              ", 0 <= n_failing <= N - 2 and N * ld * 4 B < 2 GiB (svoc.ops.lest_route)");
  TORCH_CHECK(fast_work_words(D) * 4 < (1ll << 31), "workspace too large for 32-bit buffer offsets");
  LestParams lp{};
  FastParams& p = lp.f;
  lp.weights = weights.data_ptr<float>();
  p.values = values.data_ptr();
  p.active = lest_active(active, B, values.device());
  p.inst_stride = values.stride(0);
  p.B = (int)B; p.N = (int)N; p.D = (int)D; p.ld = (int)ld;
  p.n_failing = (int)n_failing;
  p.constrained = constrained ? 1 : 0;
  p.max_spread = (float)max_spread;
  // c1 is staged and committed only where the round succeeded (a reverted round leaves every output untouched)
  at::Tensor c1_stage = at::empty_like(c1);
  p.c1 = c1_stage.data_ptr<float>();
  p.c1_out = c1.data_ptr<float>();
  p.consensus = cons.data_ptr<float>();
  p.skew = skew.data_ptr<float>();
  p.kurt = kurt.data_ptr<float>();
  p.rel = rel.data_ptr<float>();
  p.qr = qr.data_ptr<float>();
  p.reliable = reliable.data_ptr<uint8_t>();
  p.status = status.data_ptr<int32_t>();
  at::Tensor wtmp;
  if (work.has_value() && work->defined()) {
    TORCH_CHECK(work->is_contiguous() && work->element_size() == 4 && work->device() == values.device(),
                "work: contiguous 4-byte elements on the values' device");
    TORCH_CHECK(work->numel() >= fast_work_numel(B, D), "work: needs ", fast_work_numel(B, D),
                " elements (svoc.ops.fast_work_numel)");
    p.work = (uint32_t*)work->data_ptr();
  } else {
    wtmp = at::empty({fast_work_numel(B, D)}, values.options().dtype(at::kInt));
    p.work = (uint32_t*)wtmp.data_ptr();
    p.work_fresh = 1;
  }
  p.work_pairs = (int)fast_work_pairs(D);
  p.work_stride = fast_work_words(D);
  auto stream = c10::hip::getCurrentHIPStream(values.device().index()).stream();
  const int rc = svoc_lest_round_f32(&lp, stream);
  TORCH_CHECK(rc == 0, "svoc_lest_round_f32 launch failed: ", rc);
}

// the route, for Python (svoc.ops.lest_route): tensor-less, the shape as ints
std::vector<int64_t> lest_route_op(int64_t storage, int64_t N, int64_t D, int64_t ld, int64_t n_failing, bool constrained,
                                   bool legacy, int64_t mode) {
  TORCH_CHECK(N >= 1 && D >= 1 && ld >= D && N < (1ll << 31) && ld < (1ll << 31) && n_failing < (1ll << 31) &&
                  n_failing > -(1ll << 31),
              "lest_route: 1 <= N, 1 <= D <= ld (int32)");
  const LestRoute r = lest_route({(int)storage, (int)N, (int)D, (int)ld, (int)n_failing, constrained, legacy, (int)mode, 0,
                                  kWorkCaller});
  return {r.supported, r.lane_groups, r.max_n, r.needs_work};
}

}  // namespace
}  // namespace svoc

TORCH_LIBRARY_FRAGMENT(svoc, m) {
  m.def(
      "lest_round(Tensor values, Tensor? active, int D, int n_failing, bool constrained, float max_spread, "
      "Tensor weights, Tensor(a!) c1, Tensor(b!) consensus, Tensor(c!) skew, Tensor(d!) kurt, Tensor(e!) rel, "
      "Tensor(f!) qr, Tensor(g!) reliable, Tensor(h!) status, Tensor? work=None) -> ()");
  m.def("lest_route(int storage, int N, int D, int ld, int n_failing, bool constrained, bool legacy, int mode) -> int[]",
        &svoc::lest_route_op);
}

TORCH_LIBRARY_IMPL(svoc, CPU, m) { m.impl("lest_round", &svoc::lest_round_cpu); }

TORCH_LIBRARY_IMPL(svoc, CUDA, m) { m.impl("lest_round", &svoc::lest_round_hip); }
