// hep_api_util.h - the error plumbing the files of the C ABI share (hep_api.cpp: sessions and inference, hep_api_train.cpp: the
// stateless training side).  hep_last_error() returns the message of the calling thread's last failing call, whichever of the
// files the call lives in: the string behind it has ONE definition (hep_api.cpp) and is only declared here.
#pragma once
#include <new>
#include <string>

#include <hip/hip_runtime.h>

#include "hep.h"

namespace hep {

__attribute__((visibility("hidden"))) extern thread_local std::string g_err;      // (internal to libhep.so: no exported symbol)
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPRET(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(HEP_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// Nothing may leave an entry point as a C++ exception (include/hep.h: "never throws"; the C# host P/Invokes these symbols, and
// ONNXRuntime - the library this one replaces - reports failures through its API, Program.cs:59-61).  Every extern "C" function
// is a function-try-block ending in one of these handlers: std::bad_alloc / length_error from a hostile weight pack, a vector
// that outgrew memory, anything else -> HEP_ERR_INTERNAL and a message in hep_last_error().
inline int hep_caught() noexcept {
  try { throw; }
  catch (const std::bad_alloc&) { try { g_err = "out of host memory (std::bad_alloc)"; } catch (...) {} }
  catch (const std::exception& e) { try { g_err = std::string("internal error: ") + e.what(); } catch (...) {} }
  catch (...) { try { g_err = "internal error: unknown C++ exception"; } catch (...) {} }
  return HEP_ERR_INTERNAL;
}
#define HEP_CATCH_INT catch (...) { return hep_caught(); }
#define HEP_CATCH_VOID catch (...) { hep_caught(); }

}  // namespace hep
