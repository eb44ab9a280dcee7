// hep_api_util.h - what the four files of the C ABI share (hep_api.cpp: sessions and everything else that takes a hep_handle; hep_api_pose.cpp:
// frame to pose - top detection, the hep_pose(s)_from_* host calls, whole-frame search; hep_api_eval.cpp: the stateless evaluation and
// visualisation toolkit; hep_api_train.cpp: the stateless training side).  hep_last_error() returns the message of the calling
// thread's last failing call, whichever file the call lives in: the string behind it has ONE definition (hep_api.cpp) and is only declared here.
#pragma once
#include <algorithm>
#include <new>
#include <string>
#include <utility>

#include <hip/hip_runtime.h>

#include "hep.h"

namespace hep {

__attribute__((visibility("hidden"))) extern thread_local std::string g_err;      // (internal to libhep.so: no exported symbol)
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPRET(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(HEP_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define CHECKED(x) do { if (int rc_ = (x)) return rc_; } while (0)      // a refused check ends the entry point with the check's code

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

// The check vocabulary: what an entry point refuses before its first HIP call, each wording once.  A Check holds the prefix of the entry
// point's messages ("hep_draw_poses_device: ", "augment: ", "": it must outlive the Check); a member reads host memory only and, on a refusal,
// sets the message and returns the code (0: passed).  A check only one entry point makes is worded there, through fail().  (Hidden: no new export.)
struct __attribute__((visibility("hidden"))) Check {
  const char* who;
  int fail(int code, const std::string& text) const { return hep::fail(code, who + text); }
  int ptrs(std::initializer_list<std::pair<const void*, const char*>> ps) const {      // the first NULL of {pointer, name}
    for (const auto& p : ps) if (!p.first) return fail(HEP_ERR_INVALID, std::string(p.second) + " is NULL");
    return 0;
  }
  int range(const char* name, int64_t v, int64_t lo, int64_t hi, int code = HEP_ERR_INVALID, const char* hi_text = nullptr) const {      // hi_text: a limit that is another argument ("rows")
    return v >= lo && v <= hi ? 0 : fail(code, std::string(name) + " outside " + std::to_string(lo) + ".." + (hi_text ? std::string(hi_text) : std::to_string(hi)));
  }
  int at_least(const char* name, int64_t v, int64_t lo) const { return v >= lo ? 0 : fail(HEP_ERR_INVALID, std::string(name) + " must be >= " + std::to_string(lo)); }
  int frame(int height, int width, bool brackets = false) const {      // the sizes the image kernels are built for; brackets: the training side's wording
    if (height >= 16 && height <= 4096 && width >= 16 && width <= 4096) return 0;
    return fail(HEP_ERR_UNSUPPORTED, std::string("height and width must be in ") + (brackets ? "[16, 4096]" : "16..4096"));
  }
  int labels(int num_labels) const { return range("num_labels", num_labels, 1, 63); }      // SCORE_MAX_LABELS (hep_eval.h; asserted in hep_api_eval.cpp)
  int max_points(int n, int code) const { return n >= 1 && n <= 1024 ? 0 : fail(code, "max_points must be in 1..1024 (the reference uses 1000)"); }
  int aligned(const void* p, int bytes, const char* what) const {
    return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0 ? 0 : fail(HEP_ERR_INVALID, std::string(what) + " must be " + std::to_string(bytes) + "-byte aligned");
  }
  int workspace(const void* p, int64_t have, int64_t need, const char* query) const {      // query: the hep_X_workspace_bytes function that states `need`
    if (int rc = aligned(p, 16, "workspace")) return rc;
    return have >= need ? 0 : fail(HEP_ERR_INVALID, std::string("workspace too small (") + query + ")");
  }
  // a host start table [num_labels + 1], label l owning [start[l], start[l + 1]) of `count` entries: it starts at 0 or above, every label owns at
  // least one `noun` and at most `most` (0: no limit), it ends inside count
  int start_table(const char* name, const int32_t* start, int num_labels, int count, int most, const char* noun = "entry") const {
    const std::string t = name;
    if (start[0] < 0) return fail(HEP_ERR_INVALID, t + " starts below 0");
    for (int l = 0; l < num_labels; l++) {
      if (start[l + 1] <= start[l]) return fail(HEP_ERR_INVALID, t + " must increase (label " + std::to_string(l) + " has no " + noun + ")");
      if (most && start[l + 1] - start[l] > most) return fail(HEP_ERR_INVALID, t + ": label " + std::to_string(l) + " has more than " + std::to_string(most) + " entries");
    }
    return start[num_labels] > count ? fail(HEP_ERR_INVALID, t + " ends past the array") : 0;
  }
};

// preprocess_image's geometry (colibri_common.py:631-642, generators/common.py:576-607): scale = size / longer side; that side becomes size, the
// other int(side * scale); with cv2.resize's explicit size the per-axis inverse scale is src / dst.  false: the resized frame does not fit size x size
struct ResizeGeom { int resize, nh, nw; double scale, inv_scale_x, inv_scale_y; };
__attribute__((visibility("hidden"))) inline bool resize_geometry(int height, int width, int size, ResizeGeom* g) {
  const int side = std::max(height, width);
  g->resize = side != size; g->scale = (double)size / side;
  g->nh = height > width ? size : (int)(height * g->scale);
  g->nw = height > width ? (int)(width * g->scale) : size;
  if (!g->resize) { g->nh = height; g->nw = width; }
  if (g->nh > size || g->nw > size || g->nh < 1 || g->nw < 1) return false;
  g->inv_scale_x = (double)width / g->nw; g->inv_scale_y = (double)height / g->nh;
  return true;
}

}  // namespace hep
