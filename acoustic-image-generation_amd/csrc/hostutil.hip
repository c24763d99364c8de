// What libacimg offers beside its operators: acimg_version, acimg_last_error (the per-thread text that fail() in common.hpp
// leaves), acimg_zero (an asynchronous memset), acimg_spin with spin_kernel (one wave that holds a stream busy for a number of
// shader-clock cycles: acimg/ops.py's stream-overlap probe), and acimg_crc32c - CRC-32C (Castagnoli), the checksum TensorFlow's
// checkpoint bundles (tensor_bundle.cc) and TFRecord files (record_writer.cc) carry; slicing-by-8 tables (acimg/tfio.py).
#include "common.hpp"

namespace acimg {

__global__ void spin_kernel(unsigned long long cycles, unsigned* out) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    unsigned long long t = t0;
    while (t - t0 < cycles) {          // every wave reaches the exit: the clock only moves forward
        __builtin_amdgcn_s_sleep(32);
        t = __builtin_amdgcn_s_memtime();
    }
    if (threadIdx.x == 0 && out) out[0] = (unsigned)(t - t0);
}

namespace {
struct Crc32cTables {
    uint32_t t[8][256];
    Crc32cTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
    }
};
}  // namespace

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_version(void) { return ACIMG_VERSION; }

int acimg_last_error(char* buf, size_t len) {
    if (!buf || len == 0) return ACIMG_EINVAL;
    strncpy(buf, err_buf(), len - 1);
    buf[len - 1] = 0;
    return ACIMG_OK;
}

int acimg_zero(void* ptr, size_t bytes, void* stream) {
    hipError_t e = hipMemsetAsync(ptr, 0, bytes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "zero: %s", hipGetErrorString(e));
    return ACIMG_OK;
}

int acimg_spin(uint64_t cycles, void* out, void* stream) {
    if (cycles > 0xFFFFFFFFull) return fail(ACIMG_EINVAL, "spin: at most 2^32 cycles");
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)cycles,
                       static_cast<unsigned*>(out));
    return check_launch("spin");
}

uint32_t acimg_crc32c(const void* data, size_t n, uint32_t crc) {
    static const Crc32cTables T;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = ~crc;
    while (n && (reinterpret_cast<uintptr_t>(p) & 7)) {
        c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
        --n;
    }
    while (n >= 8) {
        uint64_t v;
        memcpy(&v, p, 8);
        v ^= c;
        c = T.t[7][v & 0xFF] ^ T.t[6][(v >> 8) & 0xFF] ^ T.t[5][(v >> 16) & 0xFF] ^ T.t[4][(v >> 24) & 0xFF] ^
            T.t[3][(v >> 32) & 0xFF] ^ T.t[2][(v >> 40) & 0xFF] ^ T.t[1][(v >> 48) & 0xFF] ^ T.t[0][v >> 56];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

}  // extern "C"
