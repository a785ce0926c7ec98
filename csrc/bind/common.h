// Python bindings for the MNIST HIP kernels (torch extension `_kernels`), one unit per subsystem:
// what every unit of csrc/bind/ shares.
//
// Every entry point validates device, dtype, contiguity and that each buffer is
// large enough for the indices the kernel will form, BEFORE launching: a
// mis-sized operand must raise here, never fault on the GPU.  Launches go to
// the caller's current HIP stream (so they are hipGraph-capturable and honour
// torch.cuda.stream contexts).
#pragma once
#include <algorithm>
#include <cctype>
#include <cmath>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/launchers.h"

// each unit registers its own names (module.cpp calls them in this order)
void bind_layers(py::module_& m);
void bind_input(py::module_& m);
void bind_loss(py::module_& m);
void bind_optimizer(py::module_& m);
void bind_fused_conv(py::module_& m);
void bind_f32(py::module_& m);

namespace {   // a private copy per unit: the checks stay inlined into the wrappers

using at::Tensor;
using c10::optional;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check(const Tensor& t, at::ScalarType dt, int64_t need, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
  TORCH_CHECK(need >= 0 && t.numel() >= need, name, ": needs ", need, " elements, has ", t.numel());
}

int64_t span(int64_t rows, int64_t ld, int64_t cols) { return rows <= 0 ? 0 : (rows - 1) * ld + cols; }

template <class T>
T* P(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }
const mnistx::bf16_t* BF(const Tensor& t) { return reinterpret_cast<const mnistx::bf16_t*>(t.data_ptr()); }
mnistx::bf16_t* BFm(const Tensor& t) { return reinterpret_cast<mnistx::bf16_t*>(t.data_ptr()); }

void hip_ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " launch failed: ", hipGetErrorString(e));
}

// an optional tensor argument that was passed and is not an undefined tensor
bool has(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

bool aligned(const void* p, int64_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }
bool aligned(const Tensor& t, int64_t n) { return aligned(t.data_ptr(), n); }

// the Feistel domain of a batch permutation (perm.h): 2 h bits must cover the N rows
void perm_domain(const char* who, int64_t N, int64_t h) {
  TORCH_CHECK(N > 0 && h >= 1 && h <= 31 && (1ll << (2 * h)) >= N, who, ": bad domain");
}

}  // namespace
