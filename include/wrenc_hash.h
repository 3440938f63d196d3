/* wrenc_hash.h -- the decoded picture hash (H.274 / VSEI decoded picture hash SEI, payload type 132) as both libraries
 * name it: the device takes it of the reconstruction it holds (wrenc_gpu.h, wrenc_gpu_download_hashes), the host writer
 * takes it of planes in host memory and frames the SEI message (wrenc_bitstream_hash.h).  Host only, plain C.
 *
 * 8-bit 4:2:0: three components, each hashed over its CODED plane (W x H luma, W/2 x H/2 chroma) in raster order, one
 * byte per sample -- the decoded picture before the conformance window crops it.
 *   MD5       RFC 1321 over the plane's bytes; the 16 digest bytes in digest order.
 *   CRC       register 0xFFFF, polynomial 0x1021, bits MSB first, over the plane's bytes followed by 16 zero bits:
 *             crc = ((crc << 1 | bit) & 0xFFFF) ^ (msb ? 0x1021 : 0) per bit; written u(16).
 *   checksum  sum of data[y][x] ^ (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8) modulo 2^32, x and y inside the
 *             component's own plane; written u(32). */
#ifndef WRENC_HASH_H
#define WRENC_HASH_H

#include <stdint.h>

enum { WRENC_HASH_MD5 = 0, WRENC_HASH_CRC = 1, WRENC_HASH_CHECKSUM = 2 }; /* dph_sei_hash_type */

/* Y, Cb, Cr: the bytes of each component exactly as they go into the SEI message -- MD5 16 bytes, CRC 2, checksum 4,
 * big-endian; the rest is zero. */
typedef struct wrenc_picture_hash {
    uint8_t value[3][16];
} wrenc_picture_hash;

#endif /* WRENC_HASH_H */
