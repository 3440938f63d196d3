// picture_hash.cpp -- the C ABI of include/wrenc_bitstream_hash.h: the decoded picture hash (H.274 decoded picture hash
// SEI) of planes in host memory, each hash written literally from its definition, and the SEI's NAL unit.
#include "../../../include/wrenc_bitstream_hash.h"
#include "slice_data.h"

#include <cstring>

using namespace wrenc_host;

namespace {

// RFC 1321, section 3.4: the per-step shifts and T[i] = floor(2^32 |sin(i + 1)|)
const int kMd5Shift[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9,  14, 20, 5, 9,
                           14, 20, 5, 9,  14, 20, 5, 9,  14, 20, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23,
                           4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
const uint32_t kMd5T[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1,
    0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453,
    0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942,
    0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05,
    0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d,
    0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};

void md5_block(uint32_t st[4], const uint8_t* p) {
    uint32_t m[16];
    for (int i = 0; i < 16; ++i) m[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        int g;
        if (i < 16) {
            f = (b & c) | (~b & d);
            g = i;
        } else if (i < 32) {
            f = (d & b) | (~d & c);
            g = (5 * i + 1) & 15;
        } else if (i < 48) {
            f = b ^ c ^ d;
            g = (3 * i + 5) & 15;
        } else {
            f = c ^ (b | ~d);
            g = (7 * i) & 15;
        }
        const uint32_t v = a + f + kMd5T[i] + m[g];
        a = d;
        d = c;
        c = b;
        b += v << kMd5Shift[i] | v >> (32 - kMd5Shift[i]);
    }
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
}

void md5(const uint8_t* data, size_t n, uint8_t digest[16]) {
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    size_t at = 0;
    for (; at + 64 <= n; at += 64) md5_block(st, data + at);
    // the rest, the bit 1, zeros up to 56 mod 64 and the length in bits, 64-bit little-endian
    uint8_t tail[128] = {};
    const size_t rest = n - at;
    memcpy(tail, data + at, rest);
    tail[rest] = 0x80;
    const size_t total = rest + 9 <= 64 ? 64 : 128;
    const uint64_t bits = (uint64_t)n * 8;
    for (int i = 0; i < 8; ++i) tail[total - 8 + (size_t)i] = (uint8_t)(bits >> (8 * i));
    md5_block(st, tail);
    if (total == 128) md5_block(st, tail + 64);
    for (int i = 0; i < 16; ++i) digest[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}

uint32_t crc(const uint8_t* data, size_t n) {
    uint32_t crc = 0xFFFF;
    const auto step = [&crc](uint32_t bit) {
        const uint32_t msb = (crc >> 15) & 1;
        crc = ((crc << 1 | bit) & 0xFFFF) ^ (msb ? 0x1021u : 0u);
    };
    for (size_t i = 0; i < n; ++i)
        for (int b = 7; b >= 0; --b) step((data[i] >> b) & 1u);
    for (int b = 0; b < 16; ++b) step(0);
    return crc;
}

uint32_t checksum(const uint8_t* data, int w, int h) {
    uint32_t sum = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            sum += (uint32_t)(data[(size_t)y * w + x] ^ (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8));
    return sum;
}

int value_bytes(int hash_type) {
    return hash_type == WRENC_HASH_MD5 ? 16 : (hash_type == WRENC_HASH_CRC ? 2 : (hash_type == WRENC_HASH_CHECKSUM ? 4 : 0));
}

} // namespace

extern "C" {

int wrenc_bs_picture_hash(int width, int height, int hash_type, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                          wrenc_picture_hash* out) {
    if (!value_bytes(hash_type) || !y || !cb || !cr || !out || width < 32 || height < 32 || width % 32 || height % 32 ||
        width > 16384 || height > 16384)
        return WRENC_BS_EINVAL;
    const uint8_t* plane[3] = {y, cb, cr};
    memset(out, 0, sizeof(*out));
    for (int p = 0; p < 3; ++p) {
        const int w = p ? width / 2 : width, h = p ? height / 2 : height;
        uint8_t* v = out->value[p];
        if (hash_type == WRENC_HASH_MD5) {
            md5(plane[p], (size_t)w * h, v);
        } else if (hash_type == WRENC_HASH_CRC) {
            const uint32_t c = crc(plane[p], (size_t)w * h);
            v[0] = (uint8_t)(c >> 8);
            v[1] = (uint8_t)c;
        } else {
            const uint32_t s = checksum(plane[p], w, h);
            for (int i = 0; i < 4; ++i) v[i] = (uint8_t)(s >> (24 - 8 * i));
        }
    }
    return WRENC_BS_OK;
}

int wrenc_bs_write_hash_sei(int hash_type, const wrenc_picture_hash* hash, uint8_t* out, size_t cap, size_t* len) {
    const int nb = value_bytes(hash_type);
    if (!nb || !hash) return WRENC_BS_EINVAL;
    std::vector<uint8_t> payload;
    payload.push_back(132);                    // payload_type: decoded picture hash
    payload.push_back((uint8_t)(2 + 3 * nb));  // payload_size
    payload.push_back((uint8_t)hash_type);     // dph_sei_hash_type
    payload.push_back(0);                      // dph_sei_single_component_flag = 0, dph_sei_reserved_zero_7bits
    for (int p = 0; p < 3; ++p) payload.insert(payload.end(), hash->value[p], hash->value[p] + nb);
    payload.push_back(0x80);                   // rbsp_trailing_bits
    std::vector<uint8_t> stream;
    append_nal(stream, 0, NAL_SUFFIX_SEI, 0, payload);
    if (len) *len = stream.size();
    if (!out || cap < stream.size()) return WRENC_BS_ENOSPC;
    memcpy(out, stream.data(), stream.size());
    return WRENC_BS_OK;
}

} // extern "C"
