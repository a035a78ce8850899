// Host harness for weath3rb0i_amd/csrc/w3_crc.h (tests/test_crc_cpu.py): the CRC-32 arithmetic and the per-lane piece of k_crc32_slices,
// compiled for the CPU.  A segment's CRC is computed the way the two kernels do it — cut into slices, every slice as a loop over the 64
// "lanes" of a wavefront whose shares are xored and finished, the slices' CRCs folded — and printed; the test compares with zlib.
//   crc_lanes <blob file> <case file>      one case per line, one answer (8 hex digits) per line
//     known                 crc32_ref("123456789") and crc32_ref("")   (two answers)
//     ref <off> <len>       crc32_ref of blob[off, off + len)
//     wave <off> <len> <a>  the lane form of blob[off, off + len), copied to an address that is a (0 .. 15) past a 16-byte boundary
//     guard <off> <len> <e> the lane form with the copy flush against an inaccessible page: e = 0 the buffer starts at the page start
//                           (a read before it is a SIGSEGV), e = 1 it ends at the page end (a read past it is one)
//     comb <a> <b> <len>    crc32_combine(a, b, len), a and b in hex, len in decimal (up to 2^63)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

#define W3_HD static inline
#include "../../weath3rb0i_amd/csrc/w3_crc.h"

// what k_crc32_slices + k_crc32_fold compute for one segment
static uint32_t segment_crc(const uint8_t *p, uint32_t len) {
    const uint32_t ns = w3::crc_slices_of(len);
    std::vector<uint32_t> sc(ns ? ns : 1);
    for (uint32_t j = 0; j < ns; j++) {
        const uint32_t so = j * W3_CRC_SLICE, sl = len - so < W3_CRC_SLICE ? len - so : W3_CRC_SLICE;
        const w3::CrcSlicePlan pl = w3::crc_slice_plan(p + so, sl);
        uint32_t x = 0;
        for (uint32_t lane = 0; lane < 64; lane++) x ^= w3::crc_slice_lane(pl, p + so, lane);
        sc[j] = w3::crc_slice_finish(pl, x);
    }
    return w3::crc_fold(sc.data(), len);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: crc_lanes <blob> <cases>\n"); return 2; }
    std::vector<uint8_t> blob;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        blob.resize((size_t)n);
        if (n && fread(blob.data(), 1, (size_t)n, f) != (size_t)n) { perror("read"); return 2; }
        fclose(f);
    }
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    const size_t gpages = (4096 + page - 1) / page + 1;   // room for the guarded cases (up to 4 KiB)
    uint8_t *m = (uint8_t *)mmap(nullptr, (gpages + 2) * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) { perror("mmap"); return 2; }
    if (mprotect(m, page, PROT_NONE) || mprotect(m + (gpages + 1) * page, page, PROT_NONE)) { perror("mprotect"); return 2; }
    uint8_t *lo = m + page, *hi = m + (gpages + 1) * page;
    FILE *cf = fopen(argv[2], "r");
    if (!cf) { perror(argv[2]); return 2; }
    char line[256];
    while (fgets(line, sizeof line, cf)) {
        unsigned long long a = 0, b = 0, c = 0;
        if (!strncmp(line, "known", 5)) {
            printf("%08x\n%08x\n", w3::crc32_ref((const uint8_t *)"123456789", 9), w3::crc32_ref((const uint8_t *)"", 0));
        } else if (sscanf(line, "ref %llu %llu", &a, &b) == 2) {
            if (a + b > blob.size()) return 2;
            printf("%08x\n", w3::crc32_ref(blob.data() + a, (size_t)b));
        } else if (sscanf(line, "wave %llu %llu %llu", &a, &b, &c) == 3) {
            if (a + b > blob.size() || c > 15) return 2;
            // a heap block of its own that ENDS with the data, so that a sanitizer build sees every read past it; the `a` bytes in front
            // of the data hold other values, so a read before it changes the answer
            uint8_t *raw = nullptr;
            if (posix_memalign((void **)&raw, 16, (size_t)(c + b) ? (size_t)(c + b) : 1)) return 2;
            memset(raw, 0xA5, (size_t)c);
            if (b) memcpy(raw + c, blob.data() + a, (size_t)b);
            printf("%08x\n", segment_crc(raw + c, (uint32_t)b));
            free(raw);
        } else if (sscanf(line, "guard %llu %llu %llu", &a, &b, &c) == 3) {
            if (a + b > blob.size() || b > 4096) return 2;
            uint8_t *p = c ? hi - b : lo;
            if (b) memcpy(p, blob.data() + a, (size_t)b);
            printf("%08x\n", segment_crc(p, (uint32_t)b));
        } else if (sscanf(line, "comb %llx %llx %llu", &a, &b, &c) == 3) {
            printf("%08x\n", w3::crc32_combine((uint32_t)a, (uint32_t)b, c));
        } else {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    fclose(cf);
    return 0;
}
