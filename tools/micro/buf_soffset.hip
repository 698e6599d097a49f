// Is the scalar offset of a raw buffer access part of the hardware range check?  (gfx950 semantics probe)
// A descriptor covers the first N floats of an allocation of 4 N floats; everything a line below can touch lies inside that allocation, whichever rule holds.
#include <hip/hip_runtime.h>
#include <cstdio>
constexpr int N = 64;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(float* p) { return __builtin_amdgcn_make_buffer_rsrc(p, 0, N * 4, 0x00020000); }
__global__ void probe(float* src, float* dst, float* out) {
    const __amdgpu_buffer_rsrc_t r = rsrc(src), w = rsrc(dst);
    uint4 v[4];
    v[0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (N - 4) * 4, 16, 0));      // lane offset inside, lane + scalar offset = N .. N + 3
    v[1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, 0, N * 4, 0));             // scalar offset alone reaches the end
    v[2] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (N - 1) * 4, 16, 0));      // the +16 half of a unit whose first word is the last of the buffer
    v[3] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (N - 2) * 4, 0, 0));       // no scalar offset: straddles word by word
    for (int i = 0; i < 4; ++i) { out[4 * i] = __uint_as_float(v[i].x); out[4 * i + 1] = __uint_as_float(v[i].y); out[4 * i + 2] = __uint_as_float(v[i].z); out[4 * i + 3] = __uint_as_float(v[i].w); }
    out[16] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, 8, N * 4, 0));           // one word, as the residual loads
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, 7.f), w, 8, (N + 1) * 4, 0);           // lane offset inside, scalar offset a "channel" past the end: dst[N + 3]
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, 9.f), w, 8, 4, 0);                     // both inside: dst[3]
}
int main() {
    float h[4 * N]; for (int i = 0; i < 4 * N; ++i) h[i] = 100.f + i;
    float *s, *d, *o; hipMalloc(&s, sizeof(h)); hipMalloc(&d, sizeof(h)); hipMalloc(&o, 32 * 4);
    hipMemcpy(s, h, sizeof(h), hipMemcpyHostToDevice); hipMemset(d, 0, sizeof(h)); hipMemset(o, 0, 32 * 4);
    probe<<<1, 1>>>(s, d, o);
    float r[32], t[4 * N];
    if (hipMemcpy(r, o, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(t, d, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error\n"); return 1; }
    const char* what[4] = {"voff N-4, soff 16", "voff 0, soff 4N", "voff N-1, soff 16", "voff N-2, soff 0"};
    for (int i = 0; i < 4; ++i) printf("load b128 %-18s: %g %g %g %g\n", what[i], r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
    printf("load b32  voff 2, soff 4N   : %g   (src[N + 2] = %g)\n", r[16], h[N + 2]);
    printf("store b32 voff 2, soff 4(N+1): dst[N + 3] = %g (7: stored, 0: dropped); control dst[3] = %g (9)\n", t[N + 3], t[3]);
    printf("scalar offset is %s the range check\n", (r[0] == 0.f && r[4] == 0.f && r[16] == 0.f && t[N + 3] == 0.f) ? "PART OF" : (r[0] == h[N] && t[N + 3] == 7.f) ? "EXCLUDED FROM" : "?? (mixed)");
    return 0;
}
