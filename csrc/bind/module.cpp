// _kernels: the module itself, the process-level hooks that belong to no subsystem, then every unit.
#include "bind/common.h"

PYBIND11_MODULE(_kernels, m) {
  m.doc() = "MI355X (gfx950) HIP kernels for the MNIST trainer";
  m.attr("ARCH") = "gfx950";
  // test hook: cap every persistent kernel's grid (0 = off) so small-batch oracle tests run
  // the multi-iteration (several tiles per block) paths the benchmark batches run
  m.def("set_grid_cap", [](int64_t n) { mnistx::set_grid_cap((int)n); });
  m.def("grid_cap", []() { return (int64_t)mnistx::grid_cap(); });
  m.def("set_reserve_cus", [](int64_t n) { mnistx::set_reserve_cus((int)n); });
  m.def("reserve_cus", []() { return (int64_t)mnistx::reserve_cus(); });
  // pin / unpin host memory the caller mapped itself (the PS shm data plane's slots, so the
  // worker's gradient / parameter copies are DMA, not staged through a bounce buffer)
  m.def("host_register", [](uintptr_t addr, int64_t nbytes) {
    return hipHostRegister((void*)addr, (size_t)nbytes, hipHostRegisterDefault) == hipSuccess;
  });
  m.def("host_unregister", [](uintptr_t addr) { return hipHostUnregister((void*)addr) == hipSuccess; });
  m.def("clock_mark", [](Tensor out, int64_t slot) {
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && slot >= 0 &&
                    slot < out.numel(), "clock_mark: int64 GPU buffer with the slot in range");
    hip_ok(mnistx::clock_mark((uint64_t*)out.data_ptr<int64_t>(), (int)slot, cur_stream()), "clock_mark");
  });
  m.def("coresidency_probe", [](Tensor out, int64_t blocks, int64_t threads, int64_t lds_bytes, int64_t spin_ticks) {
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && out.numel() >= 2 * blocks,
                "coresidency_probe: int64 GPU buffer of 2 * blocks stamps");
    hip_ok(mnistx::coresidency_probe((uint64_t*)out.data_ptr<int64_t>(), (int)blocks, (int)threads, (int)lds_bytes,
                                     (int)spin_ticks, cur_stream()), "coresidency_probe");
  });
  bind_layers(m);
  bind_input(m);
  bind_loss(m);
  bind_optimizer(m);
  bind_fused_conv(m);
  bind_f32(m);
}
