// szn_runtime.hip -- what every other source of libszn_hip.so links against: the error text, the last-kernel / column-sum / work-fraction
// notes, the knob table, library and device info, CU-masked streams.  No kernels.
#include "szn_common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

// ---- error plumbing -----------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void szn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* szn_last_error(void) { return g_err; }
static thread_local const char* g_last_kernel = "";
static thread_local const char* g_prev_kernel = "";
void szn_note_kernel(const char* name) { g_prev_kernel = g_last_kernel; g_last_kernel = name; }
extern "C" const char* szn_last_kernel(void) { return g_last_kernel; }
extern "C" const char* szn_prev_kernel(void) { return g_prev_kernel; }
static thread_local int g_colsum_rows = 0;
void szn_note_colsum_rows(int rows) { g_colsum_rows = rows; }
int szn_noted_colsum_rows(void) { return g_colsum_rows; }
// ---- tuning / A-B knobs: ONE table.  szn_knob() refuses names that are not listed here, so a knob cannot exist without its line in
//      DESIGN.md section 4 and its case in tests/test_gpu_knobs.py (which runs a step under every non-default value below). ----
static const char* const g_knobs[] = {
    "SZN_REGW_MINTILES", "SZN_WIDE_MINTILES", "SZN_WGT_MINTILES", "SZN_WGW_MINTILES",     // dispatch thresholds (a huge value = kernel family off)
    "SZN_WIDE_8PH", "SZN_8PH_KORD", "SZN_WIDE_ROWS", "SZN_WIDE_DIRECT", "SZN_IGEMM_DIRECT",  // which forward / dgrad tile kernel, K order, epilogue form
    "SZN_CONST_BORDER", "SZN_DGRAD_BORDER", "SZN_WGT_CB",                                 // constant-border hints
    "SZN_WGW_HALF", "SZN_WGW_STAGGER", "SZN_WGH_STAGGER", "SZN_WGW_XCD",                  // fc6's weight gradient (+ Adam)
};
static bool knob_listed(const char* name) {
    for (const char* k : g_knobs)
        if (!strcmp(k, name)) return true;
    return false;
}
int szn_knob_live(const char* name, int dflt) {
    if (!knob_listed(name)) { fprintf(stderr, "libszn_hip: unregistered knob %s\n", name); abort(); }
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
int szn_knob(const char* name, int dflt) { return szn_knob_live(name, dflt); }   // (callers cache it in a function-local static: read once per process)
extern "C" int szn_knob_count(void) { return (int)(sizeof(g_knobs) / sizeof(g_knobs[0])); }
extern "C" const char* szn_knob_name(int i) { return (i >= 0 && i < szn_knob_count()) ? g_knobs[i] : nullptr; }
static thread_local float g_work_fraction = 1.f;
void szn_note_work_fraction(float f) { g_work_fraction = f; }
float szn_noted_work_fraction(void) { return g_work_fraction; }

extern "C" int szn_version(void) { return 116; /* 0.1.16: szn_augment_affine_u8 */ }
extern "C" int szn_device_info(int device, szn_device_info_t* out) {
    if (!out) SZN_FAIL(SZN_ERR_ARG, "device_info: null output");
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, device);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "device_info: %s", hipGetErrorString(e));
    memset(out, 0, sizeof(*out));
    strncpy(out->name, p.name, sizeof(out->name) - 1);
    strncpy(out->arch, p.gcnArchName, sizeof(out->arch) - 1);
    out->compute_units = p.multiProcessorCount;
    out->wavefront = p.warpSize;
    out->lds_bytes_per_block = (int)p.sharedMemPerBlock;
    out->hbm_bytes = (int64_t)p.totalGlobalMem;
    out->clock_mhz = p.clockRate / 1000;
    return SZN_OK;
}

// A stream whose kernels only run on the compute units of `mask` (bit i of word i / 32 = CU i; hipExtStreamCreateWithCUMask).  The
// engine confines the HBM-bound weight gradient + Adam step of fc6 in a ONE-image step to part of the chip with it, so that the few-tile
// dgrads of conv5_x .. conv3_x run beside it instead of queueing for its LDS (models._Engine._side_stream).
extern "C" int szn_stream_create_cu_mask(int n_words, const uint32_t* mask, szn_stream_t* out) {
    if (!out || !mask || n_words <= 0) SZN_FAIL(SZN_ERR_ARG, "stream_create_cu_mask: null / empty argument");
    bool any = false;
    for (int i = 0; i < n_words; ++i) any = any || mask[i] != 0u;
    if (!any) SZN_FAIL(SZN_ERR_ARG, "stream_create_cu_mask: the mask selects no compute unit");
    hipStream_t s = nullptr;
    hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "stream_create_cu_mask: %s", hipGetErrorString(e));
    *out = (szn_stream_t)s;
    return SZN_OK;
}
extern "C" int szn_stream_destroy(szn_stream_t stream) {
    if (!stream) SZN_FAIL(SZN_ERR_ARG, "stream_destroy: null stream");
    hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) SZN_FAIL(SZN_ERR_LAUNCH, "stream_destroy: %s", hipGetErrorString(e));
    return SZN_OK;
}
