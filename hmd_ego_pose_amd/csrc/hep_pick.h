// hep_pick.h - a Pick says which device function a launch runs and how.  Every kernel family has ONE function *_pick(const Args&)
// next to its kernels that holds the conditions choosing an instantiation; launch_* launches the pick, hep_kernel_symbol prints
// its name, plan_session refuses a plan with an empty pick and build_session raises the dynamic-LDS limit of the picks of its plan.
// HEP_PICK spells the template argument list once: the tokens that instantiate the kernel are the tokens that print its name.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>
#include <string>

struct PickArg {      // one template argument by value: bools print as true / false, ints in decimal (an enumerator is an int)
  bool is_bool; int v;
  constexpr PickArg() : is_bool(false), v(0) {}
  constexpr PickArg(bool b) : is_bool(true), v(b) {}
  constexpr PickArg(int i) : is_bool(false), v(i) {}
};

struct Pick {
  const void* fn = nullptr;      // host-side address of the __global__ instantiation; nullptr: none is built for these arguments
  const char* base = "";         // the kernel's name without template arguments
  unsigned block = 0;            // threads per workgroup
  size_t lds = 0;                // dynamic LDS bytes of the launch
  int max_lds = 0;               // hipFuncAttributeMaxDynamicSharedMemorySize the function needs (0: the default limit is enough)
  PickArg args[8]; int nargs = 0;
  Pick() {}
  Pick(const void* f, const char* b, unsigned blk, size_t l, int ml, std::initializer_list<PickArg> il) : fn(f), base(b), block(blk), lds(l), max_lds(ml) {
    for (const PickArg& x : il) args[nargs++] = x;
  }
  // base<a, b, ...> as rocprofv3 --kernel-trace prints the instantiation (trailing defaulted arguments the pick left out are left out)
  std::string name() const {
    std::string n = base;
    for (int i = 0; i < nargs; i++) { n += i ? ", " : "<"; n += args[i].is_bool ? (args[i].v ? "true" : "false") : std::to_string(args[i].v); }
    if (nargs) n += '>';
    return n;
  }
  // what the triple-chevron stub does: the kernel's parameters, in order and of exactly the kernel's parameter types
  template <class... A> void launch(dim3 grid, hipStream_t s, const A&... a) const {
    void* p[] = {const_cast<void*>(static_cast<const void*>(&a))...};
    (void)hipLaunchKernel(fn, grid, dim3(block), p, lds, s);
  }
};

#define HEP_PICK(block, lds, max_lds, kernel, ...) \
  Pick(reinterpret_cast<const void*>(&kernel<__VA_ARGS__>), #kernel, (unsigned)(block), (size_t)(lds), (int)(max_lds), {__VA_ARGS__})
