// Host code the four file codecs' entries share (jpeg_api.cpp, jpeg_decode_api.cpp, png_api.cpp, png_decode_api.cpp): PNG's CRC-32 and
// big-endian words, and the argument checks every encode and decode entry makes, each with the entry's name in front of one text.
#pragma once
#include "api_common.h"

namespace nesr {
namespace codec {

inline uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline void be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

inline int check_order(const char* who, int order) {
    if (order != NESR_ORDER_RGB && order != NESR_ORDER_BGR) return set_error(NESR_ERR_ARG, std::string(who) + ": order must be NESR_ORDER_RGB or NESR_ORDER_BGR");
    return NESR_OK;
}

inline int check_row_stride(const char* who, int64_t row_bytes, int64_t row) {
    if (row_bytes < row) return set_error(NESR_ERR_ARG, std::string(who) + ": the row stride is smaller than a row");
    return NESR_OK;
}

inline int check_scratch(const char* who, const void* ptr, size_t have, size_t need) {
    if (have < need) return set_error(NESR_ERR_ARG, std::string(who) + ": scratch of " + std::to_string(have) + " bytes, " + std::to_string(need) + " needed");
    if (reinterpret_cast<uintptr_t>(ptr) & 15) return set_error(NESR_ERR_ARG, std::string(who) + ": the scratch must be 16-byte aligned");
    return NESR_OK;
}

// the length, status or segment words the kernels write or read whole: `name` must be `bytes`-aligned
inline int check_word_alignment(const char* who, const char* name, const void* ptr, int bytes) {
    if (reinterpret_cast<uintptr_t>(ptr) & (uintptr_t)(bytes - 1))
        return set_error(NESR_ERR_ARG, std::string(who) + ": " + name + " must be " + std::to_string(bytes) + "-byte aligned");
    return NESR_OK;
}

}  // namespace codec
}  // namespace nesr
