/* wrenc_bitstream_hash.h -- the decoded picture hash SEI: the hashes of planes in host memory and the framed NAL unit.
 *
 * A stream that carries the hash of every decoded picture verifies itself in any conforming decoder.  The definitions
 * are in wrenc_hash.h; the device takes the same hashes of the reconstruction it holds (wrenc_gpu.h,
 * wrenc_gpu_download_hashes), so the planes need not cross the bus for it.  Status codes and conventions are those of
 * wrenc_bitstream.h.  (A header of its own, like wrenc_bitstream_qp.h.) */
#ifndef WRENC_BITSTREAM_HASH_H
#define WRENC_BITSTREAM_HASH_H

#include "wrenc_bitstream.h"
#include "wrenc_hash.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The three hashes of a width x height picture (the coded size: whole 32x32 CTUs, as the writers take it) whose planes
 * lie in host memory, tightly packed: y width x height, cb and cr width/2 x height/2.  Written literally from the
 * definitions: for callers who have the reconstruction on the host, and the statement the device pass is held against.
 * WRENC_BS_EINVAL for an unknown hash_type, a size that is not whole CTUs, or a null pointer. */
int wrenc_bs_picture_hash(int width, int height, int hash_type, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                          wrenc_picture_hash* out);

/* The SEI message in a SUFFIX_SEI_NUT NAL unit of its own (type 24, layer 0, temporal id 0: header bytes 00 C1), framed
 * like every other unit (six-byte prefix, emulation prevention); it goes directly behind the picture's slice NAL unit.
 * Payload: payload_type 0x84, payload_size (50 MD5, 8 CRC, 14 checksum), dph_sei_hash_type u(8), one byte 0x00
 * (dph_sei_single_component_flag = 0 and seven reserved zero bits), the three components' values Y, Cb, Cr, and
 * rbsp_trailing_bits 0x80.  WRENC_BS_ENOSPC with the needed size in *len when cap is too small (out may then be NULL);
 * WRENC_BS_EINVAL for an unknown hash_type or a null hash. */
int wrenc_bs_write_hash_sei(int hash_type, const wrenc_picture_hash* hash, uint8_t* out, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_BITSTREAM_HASH_H */
