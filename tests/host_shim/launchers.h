// The declarations of pesr_amd/csrc/launchers.h that the host-compiled kernel files define (jpeg.hip, resize_to.hip, resize.hip,
// degrade.hip): each one's main.cpp gets its launcher from here.
#pragma once
size_t pesr_jpeg_workspace_bytes_host(const long long* desc_host, int n, int chroma);
int pesr_jpeg_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                        int chroma, const double* dct_dev, const double* quant_dev, void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_resize_to_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                  int n, int axis, const void* tables_dev, long table_words, hipStream_t stream);
int pesr_imresize_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                 int n_images, int axis, int s, int up, const double* weights_host, hipStream_t stream);
int pesr_degrade_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                           int s, int K, const double* bank_dev, int n_kernels, hipStream_t stream);
