// torch.ops.svoc.bootstrap_oracles: fused sentiment scores -> stochastic oracle predictions.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <vector>

#include "svoc/bootstrap.hpp"
#include "svoc/ops.hpp"

extern "C" int svoc_bootstrap(const svoc::BootParams* p, hipStream_t s);

namespace svoc {
namespace {

// Every check comes before a pointer is taken.  The entries of label_idx are NOT checked here: reading them
// back would synchronise with the host, and c4 replays this op in a captured graph.  SentimentOraclePipeline
// checks their range (0 <= i < 28) where it builds the tensor.
BootParams prep(const at::Tensor& scores, const at::Tensor& label_idx, at::Tensor& out, int64_t n_failing,
                int64_t subset, int64_t seed) {
  // (the dispatcher picks the HIP implementation when ANY argument is a device tensor: a host tensor among
  // them is refused here, before a kernel could read through its pointer)
  TORCH_CHECK(label_idx.device() == scores.device() && out.device() == scores.device(),
              "bootstrap_oracles: label_idx and out must be on ", scores.device(), " (got ", label_idx.device(),
              ", ", out.device(), ")");
  TORCH_CHECK(scores.dim() == 3 && scores.size(2) == 28 && scores.scalar_type() == at::kFloat &&
              scores.is_contiguous(), "scores: float32 [W, C, 28]");
  TORCH_CHECK(label_idx.scalar_type() == at::kInt && label_idx.is_contiguous(), "label_idx: int32 [D]");
  TORCH_CHECK(out.dim() == 3 && out.scalar_type() == at::kFloat && out.is_contiguous() &&
              out.size(0) == scores.size(0) && out.size(2) == label_idx.numel(), "out: float32 [W, N, D]");
  TORCH_CHECK(scores.size(1) <= 64 && out.size(1) <= 256 && out.size(2) <= 16, "C <= 64, N <= 256, D <= 16");
  TORCH_CHECK(scores.size(1) >= 1, "bootstrap_oracles: C >= 1 (an honest oracle averages comments)");
  TORCH_CHECK(subset >= 1, "bootstrap_oracles: subset >= 1 (got ", subset, ")");
  TORCH_CHECK(n_failing >= 0 && n_failing <= out.size(1), "bootstrap_oracles: n_failing outside [0, N] (got ",
              n_failing, ")");
  BootParams p{};
  p.scores = scores.data_ptr<float>();
  p.label_idx = label_idx.data_ptr<int32_t>();
  p.out = out.data_ptr<float>();
  p.W = (int)scores.size(0); p.C = (int)scores.size(1); p.N = (int)out.size(1); p.D = (int)out.size(2);
  // (an honest oracle draws min(subset, C) comments and C <= 64: a subset beyond int range is kept as 64)
  p.n_failing = (int)n_failing; p.subset = (int)(subset < 64 ? subset : 64); p.seed = (uint64_t)seed;
  return p;
}

void bootstrap_cpu(const at::Tensor& scores, const at::Tensor& label_idx, at::Tensor out, int64_t n_failing,
                   int64_t subset, int64_t seed) {
  BootParams p = prep(scores, label_idx, out, n_failing, subset, seed);
  std::vector<int> perm(p.N);
  for (int w = 0; w < p.W; ++w) {
    boot_perm(p, w, perm.data());
    for (int j = 0; j < p.N; ++j) boot_slot(p, w, j, p.out + ((int64_t)w * p.N + perm[j]) * p.D);
  }
}

void bootstrap_hip(const at::Tensor& scores, const at::Tensor& label_idx, at::Tensor out, int64_t n_failing,
                   int64_t subset, int64_t seed) {
  TORCH_CHECK(scores.device().is_cuda(), "bootstrap_oracles: scores must be on the device of the other tensors");
  BootParams p = prep(scores, label_idx, out, n_failing, subset, seed);
  auto stream = c10::hip::getCurrentHIPStream(scores.device().index()).stream();
  const int rc = svoc_bootstrap(&p, stream);
  TORCH_CHECK(rc == 0, "svoc_bootstrap failed: ", rc);
}

}  // namespace

void register_generator_defs(torch::Library& m) {
  m.def("bootstrap_oracles(Tensor scores, Tensor label_idx, Tensor(a!) out, int n_failing, int subset, int seed) -> ()");
}
void register_generator_cpu(torch::Library& m) { m.impl("bootstrap_oracles", &bootstrap_cpu); }
void register_generator_hip(torch::Library& m) { m.impl("bootstrap_oracles", &bootstrap_hip); }

}  // namespace svoc
