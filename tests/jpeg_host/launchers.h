// The two declarations of pesr_amd/csrc/launchers.h that csrc/jpeg.hip defines, for the host build.
#pragma once
size_t pesr_jpeg_workspace_bytes_host(const long long* desc_host, int n, int chroma);
int pesr_jpeg_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                        int chroma, const double* dct_dev, const double* quant_dev, void* ws, size_t ws_bytes, hipStream_t stream);
