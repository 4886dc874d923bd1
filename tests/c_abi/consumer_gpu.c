/* The GPU leg of the compiled-C consumer: one s3r_conv_forward and one s3r_chamfer_forward driven from plain C through
 * include/s3r.h, device memory from libamdhip64 resolved with dlopen (no HIP headers: a C / cgo / JNI maintainer needs
 * only hipMalloc / hipMemcpy / hipMemset / hipDeviceSynchronize / hipFree).  tests/test_c_abi_gpu.py writes the inputs as raw
 * little-endian files, runs this, and compares the outputs with tests/golden/.
 *
 *   consumer_gpu conv <dir> <22 desc fields>    reads x.bin (halo-padded input), w.bin (torch layout), scale.bin, shift.bin;
 *                                               packs the weights on the device, runs the layer, writes y.bin
 *   consumer_gpu chamfer <dir> <B> <N> <M>      reads p.bin, q.bin; writes d1.bin d2.bin i1.bin i2.bin
 *
 * A trailing offset=<floats> carves every device buffer of the call (x, w, scale, shift, packed weights, scratch, y; the clouds and
 * the four Chamfer outputs) out of ONE hipMalloc, each block starting <floats> floats behind the end of the previous one: the way
 * a caller of an API that never allocates lays out an arena.  fp32 / int32 tensors need 4-byte alignment only (s3r.h, Conventions),
 * so offset=1 must give the results of separate allocations.
 */
#include <dlfcn.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "s3r.h"

typedef int (*malloc_fn)(void**, size_t);
typedef int (*free_fn)(void*);
typedef int (*memcpy_fn)(void*, const void*, size_t, int);
typedef int (*memset_fn)(void*, int, size_t);
typedef int (*sync_fn)(void);
static malloc_fn hip_malloc;
static free_fn hip_free;
static memcpy_fn hip_memcpy;
static memset_fn hip_memset;
static sync_fn hip_sync;
enum { H2D = 1, D2H = 2 };

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } while (0)
#define HIP(call) do { int e_ = (call); if (e_) DIE("%s -> hip error %d", #call, e_); } while (0)
#define S3R(call) do { int e_ = (call); if (e_ < 0) DIE("%s -> %d: %s", #call, e_, s3r_last_error()); } while (0)

static void* read_file(const char* dir, const char* name, size_t* bytes) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE* f = fopen(path, "rb");
    if (!f) DIE("cannot open %s", path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc((size_t)n);
    if (fread(p, 1, (size_t)n, f) != (size_t)n) DIE("short read of %s", path);
    fclose(f);
    *bytes = (size_t)n;
    return p;
}

static void write_file(const char* dir, const char* name, const void* p, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) DIE("cannot write %s", path);
    fclose(f);
}

/* device memory: one hipMalloc per buffer, or (offset=<floats>) blocks carved out of one arena at float granularity */
static long arena_off = -1;            /* floats between two blocks; < 0: no arena */
static char* arena;
static size_t arena_cap, arena_used;

static void arena_open(const size_t* bytes, int blocks) {
    if (arena_off < 0) return;
    arena_cap = 0;
    for (int i = 0; i < blocks; ++i) arena_cap += 4 * (size_t)arena_off + (bytes[i] + 3) / 4 * 4;
    HIP(hip_malloc((void**)&arena, arena_cap ? arena_cap : 4));
}

static void* dev_alloc(size_t bytes) {
    void* d = NULL;
    if (arena_off < 0) {
        HIP(hip_malloc(&d, bytes));
        return d;
    }
    arena_used += 4 * (size_t)arena_off;
    if (arena_used + bytes > arena_cap) DIE("arena of %zu bytes is too small", arena_cap);
    d = arena + arena_used;
    arena_used += (bytes + 3) / 4 * 4;
    return d;
}

static void dev_free(void* d) {
    if (arena_off < 0 && d) hip_free(d);
}

static void* to_device(const void* h, size_t bytes) {
    void* d = dev_alloc(bytes);
    HIP(hip_memcpy(d, h, bytes, H2D));
    return d;
}

static void from_device(const char* dir, const char* name, const void* d, size_t bytes) {
    void* h = malloc(bytes);
    HIP(hip_memcpy(h, d, bytes, D2H));
    write_file(dir, name, h, bytes);
    free(h);
}

static int64_t ipow(int64_t b, int e) {
    int64_t r = 1;
    while (e-- > 0) r *= b;
    return r;
}

int main(int argc, char** argv) {
    void* hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!hip) DIE("dlopen libamdhip64.so: %s", dlerror());
    hip_malloc = (malloc_fn)dlsym(hip, "hipMalloc");
    hip_free = (free_fn)dlsym(hip, "hipFree");
    hip_memcpy = (memcpy_fn)dlsym(hip, "hipMemcpy");
    hip_memset = (memset_fn)dlsym(hip, "hipMemset");
    hip_sync = (sync_fn)dlsym(hip, "hipDeviceSynchronize");
    if (!hip_malloc || !hip_free || !hip_memcpy || !hip_memset || !hip_sync) DIE("libamdhip64 lacks a runtime symbol");
    if (s3r_abi_version() != S3R_ABI_VERSION) DIE("library ABI %d != header ABI %d", s3r_abi_version(), S3R_ABI_VERSION);
    if (argc < 3) DIE("usage: consumer_gpu conv|chamfer <dir> ... [offset=<floats>]");
    const char* dir = argv[2];
    if (!strncmp(argv[argc - 1], "offset=", 7)) {
        arena_off = strtol(argv[argc - 1] + 7, NULL, 10);
        if (arena_off < 0) DIE("offset must be >= 0 floats");
        --argc;
    }

    if (!strcmp(argv[1], "conv")) {
        if (argc != 3 + 22) DIE("conv needs 22 descriptor fields");
        s3r_conv_desc d;
        int32_t* f = (int32_t*)&d;
        for (int i = 0; i < 21; ++i) f[i] = (int32_t)strtol(argv[3 + i], NULL, 10);
        d.act_param = strtof(argv[3 + 21], NULL);
        size_t nx, nw, ns, nb;
        void *hx = read_file(dir, "x.bin", &nx), *hw = read_file(dir, "w.bin", &nw);
        void *hs = read_file(dir, "scale.bin", &ns), *hb = read_file(dir, "shift.bin", &nb);
        int64_t packed_elems = 0;
        S3R(s3r_conv_packed_elems(&d, &packed_elems));
        int64_t scratch_elems = s3r_conv_scratch_elems(&d);
        if (scratch_elems < 0) DIE("scratch query: %s", s3r_last_error());
        int m = s3r_conv_out_size(&d);
        int64_t ny = (int64_t)d.batch * d.cout * ipow(m + 2 * d.out_halo, d.ndim);
        const size_t blocks[7] = {nx, nw, ns, nb, (size_t)packed_elems * 4, (size_t)scratch_elems * 4, (size_t)ny * 4};
        arena_open(blocks, 7);
        void* x = to_device(hx, nx);
        void* w = to_device(hw, nw);
        float* scale = (float*)to_device(hs, ns);
        float* shift = (float*)to_device(hb, nb);
        free(hx); free(hw); free(hs); free(hb);
        void* packed = dev_alloc((size_t)packed_elems * 4);
        S3R(s3r_conv_pack_weights(&d, (const float*)w, packed, NULL));
        float* scratch = NULL;
        if (scratch_elems) {
            scratch = (float*)dev_alloc((size_t)scratch_elems * 4);
            HIP(hip_memset(scratch, 0, (size_t)scratch_elems * 4));
        }
        void* y = dev_alloc((size_t)ny * 4);
        HIP(hip_memset(y, 0, (size_t)ny * 4));
        S3R(s3r_conv_forward(&d, x, packed, scale, shift, y, scratch, scratch_elems, NULL));
        HIP(hip_sync());
        from_device(dir, "y.bin", y, (size_t)ny * 4);
        printf("conv out_size=%d packed=%" PRId64 " scratch=%" PRId64 " y_elems=%" PRId64 " x_mod16=%d\n", m, packed_elems, scratch_elems, ny,
               (int)((uintptr_t)x & 15));
        dev_free(x);
        dev_free(w);
        dev_free(scale);
        dev_free(shift);
        dev_free(packed);
        dev_free(y);
        dev_free(scratch);
    } else if (!strcmp(argv[1], "chamfer")) {
        if (argc != 6) DIE("chamfer needs B N M");
        int B = atoi(argv[3]), N = atoi(argv[4]), M = atoi(argv[5]);
        size_t np, nq;
        void *hp = read_file(dir, "p.bin", &np), *hq = read_file(dir, "q.bin", &nq);
        if (np != (size_t)B * N * 12 || nq != (size_t)B * M * 12) DIE("cloud sizes do not match B N M");
        const size_t blocks[6] = {np, nq, (size_t)B * N * 4, (size_t)B * N * 4, (size_t)B * M * 4, (size_t)B * M * 4};
        arena_open(blocks, 6);
        float* p = (float*)to_device(hp, np);
        float* q = (float*)to_device(hq, nq);
        free(hp); free(hq);
        float* d1 = (float*)dev_alloc((size_t)B * N * 4);
        int32_t* i1 = (int32_t*)dev_alloc((size_t)B * N * 4);
        float* d2 = (float*)dev_alloc((size_t)B * M * 4);
        int32_t* i2 = (int32_t*)dev_alloc((size_t)B * M * 4);
        S3R(s3r_chamfer_forward(p, q, d1, d2, i1, i2, B, N, M, NULL));
        HIP(hip_sync());
        from_device(dir, "d1.bin", d1, (size_t)B * N * 4);
        from_device(dir, "i1.bin", i1, (size_t)B * N * 4);
        from_device(dir, "d2.bin", d2, (size_t)B * M * 4);
        from_device(dir, "i2.bin", i2, (size_t)B * M * 4);
        printf("chamfer B=%d N=%d M=%d p_mod16=%d\n", B, N, M, (int)((uintptr_t)p & 15));
        dev_free(p);
        dev_free(q);
        dev_free(d1);
        dev_free(d2);
        dev_free(i1);
        dev_free(i2);
    } else {
        DIE("unknown mode %s", argv[1]);
    }
    if (arena) hip_free(arena);
    return 0;
}
