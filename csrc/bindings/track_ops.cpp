// torch.ops.svoc.track_update: the per-oracle track record after a committed round (CPU twin + HIP launch).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "svoc/ops.hpp"
#include "svoc/track.hpp"

extern "C" int svoc_track_update(const svoc::TrackUpdate* p, hipStream_t stream);

namespace svoc {
namespace {

// Every shape, dtype and device check happens here, before any pointer is read on either backend.
TrackUpdate prep_track(const at::Tensor& active, const at::Tensor& status, const at::Tensor& reliable,
                       const at::Tensor& qr, at::Tensor& rounds, at::Tensor& flagged, at::Tensor& streak,
                       at::Tensor& score) {
  const auto dev = qr.device();
  auto chk = [&](const at::Tensor& t, const char* n) {
    TORCH_CHECK(t.device() == dev, "track_update: ", n, " must be on ", dev, " (got ", t.device(), ")");
    TORCH_CHECK(t.is_contiguous(), "track_update: ", n, " must be contiguous");
  };
  chk(active, "active"); chk(status, "status"); chk(reliable, "reliable"); chk(qr, "qr");
  chk(rounds, "rounds"); chk(flagged, "flagged"); chk(streak, "streak"); chk(score, "score");
  TORCH_CHECK(qr.dim() == 2 && (qr.scalar_type() == at::kLong || qr.scalar_type() == at::kFloat),
              "track_update: qr: int64 (exact) or fp32 (fast) [B, N]");
  const int64_t B = qr.size(0), N = qr.size(1);
  TORCH_CHECK(N >= 1 && N < (int64_t(1) << 30), "track_update: N out of range");
  TORCH_CHECK((active.scalar_type() == at::kByte || active.scalar_type() == at::kBool) && active.dim() == 1 &&
              active.numel() == B, "track_update: active: uint8/bool [B]");
  TORCH_CHECK(status.scalar_type() == at::kInt && status.dim() == 1 && status.numel() == B,
              "track_update: status: int32 [B]");
  TORCH_CHECK((reliable.scalar_type() == at::kByte || reliable.scalar_type() == at::kBool) &&
              reliable.sizes() == qr.sizes(), "track_update: reliable: uint8/bool [B, N]");
  TORCH_CHECK(rounds.scalar_type() == at::kInt && rounds.dim() == 1 && rounds.numel() == B,
              "track_update: rounds: int32 [B]");
  TORCH_CHECK(flagged.scalar_type() == at::kInt && flagged.sizes() == qr.sizes(), "track_update: flagged: int32 [B, N]");
  TORCH_CHECK(streak.scalar_type() == at::kInt && streak.sizes() == qr.sizes(), "track_update: streak: int32 [B, N]");
  TORCH_CHECK(score.scalar_type() == at::kLong && score.sizes() == qr.sizes(), "track_update: score: int64 [B, N]");
  TrackUpdate p{};
  p.B = B; p.N = (int)N; p.exact = qr.scalar_type() == at::kLong ? 1 : 0;
  if (B == 0) return p;
  p.active = (const uint8_t*)active.data_ptr();
  p.status = status.data_ptr<int32_t>();
  p.reliable = (const uint8_t*)reliable.data_ptr();
  p.qr = qr.data_ptr();
  p.rounds = rounds.data_ptr<int32_t>();
  p.flagged = flagged.data_ptr<int32_t>();
  p.streak = streak.data_ptr<int32_t>();
  p.score = score.data_ptr<int64_t>();
  return p;
}

void track_update_cpu(const at::Tensor& active, const at::Tensor& status, const at::Tensor& reliable,
                      const at::Tensor& qr, at::Tensor rounds, at::Tensor flagged, at::Tensor streak,
                      at::Tensor score) {
  TORCH_CHECK(qr.device().is_cpu(), "track_update: qr must be a host tensor here");
  const TrackUpdate p = prep_track(active, status, reliable, qr, rounds, flagged, streak, score);
  for (int64_t b = 0; b < p.B; ++b) track_update_one(p, b);
}

void track_update_hip(const at::Tensor& active, const at::Tensor& status, const at::Tensor& reliable,
                      const at::Tensor& qr, at::Tensor rounds, at::Tensor flagged, at::Tensor streak,
                      at::Tensor score) {
  // (the dispatcher comes here when ANY argument is a device tensor: a host tensor among them is refused by
  // prep_track before a kernel could read through its pointer)
  TORCH_CHECK(qr.device().is_cuda(), "track_update: qr must be on the device of the other tensors (got ",
              qr.device(), ")");
  const TrackUpdate p = prep_track(active, status, reliable, qr, rounds, flagged, streak, score);
  if (p.B == 0) return;
  const int rc = svoc_track_update(&p, c10::hip::getCurrentHIPStream(qr.device().index()).stream());
  TORCH_CHECK(rc == 0, "svoc_track_update failed: ", rc);
}

}  // namespace

void register_track_defs(torch::Library& m) {
  m.def("track_update(Tensor active, Tensor status, Tensor reliable, Tensor qr, Tensor(a!) rounds, "
        "Tensor(b!) flagged, Tensor(c!) streak, Tensor(d!) score) -> ()");
}
void register_track_cpu(torch::Library& m) { m.impl("track_update", &track_update_cpu); }
void register_track_hip(torch::Library& m) { m.impl("track_update", &track_update_hip); }

}  // namespace svoc
