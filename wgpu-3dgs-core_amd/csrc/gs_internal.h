// gs_internal.h — helpers shared by ALL host translation units of libgs3d_hip.so; free of HIP (gs_ply.cpp and gs_spz.cpp
// are also built by a plain C++ compiler).  What only the HIP units share is in gs_host.h.
#pragma once
#include "../../include/gs3d.h"

// records the thread-local error details (gs_last_error) and returns `code`
gs_status gs_fail(gs_status code, uint64_t a, uint64_t b, uint64_t c, const char *fmt, ...)
    __attribute__((format(printf, 5, 6)));

#ifdef __cplusplus
#include <string>
#include <vector>
// gs_ply.cpp, for the export path in gs_export.hip: the header gs_ply_write puts in front of n records
std::string gs_ply_header(size_t n);
// gs_spz.cpp, for the export path: what gs_spz_encode_decompressed checks and lays out before it encodes n records — the
// header, the byte offsets of the six columns, the SH coefficients per channel, the bucket of quantize_sh and the payload size
gs_status gs_spz_encode_layout(size_t n, const gs_spz_options *opt, gs_spz_header *header_out, size_t col_offset[6],
                               uint32_t *ncoef_out, uint32_t *bucket_out, size_t *bytes_out);
// gs_spz.cpp, for the device load path in gs_core.hip: validates the header of a DECOMPRESSED SPZ payload
// and its length, returns the byte offsets of the six columns (positions, alphas, colors, scales,
// rotations, sh) and the SH coefficients per channel; errors as gs_spz_decode_decompressed
gs_status gs_spz_payload_layout(const void *bytes, size_t len, gs_spz_header *header_out, size_t col_offset[6],
                                uint32_t *ncoef_out);
// gs_deflate.cpp, for the device encoder in gs_deflate.hip: the 10 header bytes in front of `body` DEFLATE bytes at out + 10
// and the trailer (CRC-32 and length of the `len` input bytes) behind them
void gs_gzip_fast_frame(uint8_t *out, size_t body, uint32_t crc, size_t len);
// ... and the CRC-32 of `len` input bytes from the CRCs of its chunks of 32768 (the last one shorter)
uint32_t gs_gzip_fast_fold_crcs(const uint32_t *crcs, size_t chunks, size_t len);
// the bounded gunzip of gs_spz_decode
gs_status gs_spz_gunzip(const void *bytes, size_t len, std::vector<uint8_t> &out);
#endif
