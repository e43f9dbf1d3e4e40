// ASAN / UBSAN harness for the host half of the device entropy decoder (vtx_jpeg_describe: markers, tables, the byte scan for
// the restart intervals' extents): mutated streams must be refused or described, with no out-of-bounds access.  Stand-alone:
//   clang++ <emulator flags> -fsanitize=address,undefined -c virtex_amd/csrc/jpeg.hip -o jpeg_asan.o
//   clang++ -fsanitize=address,undefined jpeg_describe_fuzz.cpp jpeg_asan.o tests/hipemu/obj/core.o tests/hipemu/obj/hipemu_rt.o -pthread
//   ./a.out 40000 seed1.jpg seed2.jpg ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
extern "C" int vtx_jpeg_describe(const void* data, long n, int subseq_bits, int* dinfo, void* desc, long desc_cap, void* scan_out,
                                 long scan_cap, const long* place);
static uint64_t s = 88172645463325252ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }
int main(int argc, char** argv) {
    std::vector<std::vector<uint8_t>> seeds;
    for (int i = 2; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb"); if (!f) continue;
        std::vector<uint8_t> b; uint8_t buf[4096]; size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
        fclose(f); seeds.push_back(b);
    }
    if (argc < 3 || seeds.empty()) { fprintf(stderr, "usage: %s iterations seed.jpg ...\n", argv[0]); return 2; }
    long N = atol(argv[1]), ok = 0, refused = 0;
    for (long it = 0; it < N; ++it) {
        std::vector<uint8_t> d = seeds[rnd() % seeds.size()];
        const uint32_t mode = rnd() % 100;
        if (mode < 50) { int k = 1 + rnd() % 4; for (int j = 0; j < k; ++j) d[rnd() % d.size()] = (uint8_t)rnd(); }
        else if (mode < 70) d.resize(2 + rnd() % (d.size() - 2));
        else if (mode < 85) { size_t i = rnd() % (d.size() - 4); static const uint8_t mk[] = {0xC0, 0xC4, 0xDB, 0xDA, 0xDD, 0xD3, 0xD9, 0xFF};
                              d[i] = 0xFF; d[i + 1] = mk[rnd() % 8]; }
        else { size_t i = rnd() % d.size(); int k = 1 + rnd() % 40; std::vector<uint8_t> ins(k); for (auto& x : ins) x = (uint8_t)rnd();
               d.insert(d.begin() + i, ins.begin(), ins.end()); }
        uint8_t* p = (uint8_t*)malloc(d.size()); memcpy(p, d.data(), d.size());      // exact size: a read past the end is a report
        const int bits = 128 << (rnd() % 5);
        int dinfo[8] = {0};
        if (vtx_jpeg_describe(p, (long)d.size(), bits, dinfo, nullptr, 0, nullptr, 0, nullptr) != 0) { ++refused; free(p); continue; }
        void* desc = malloc(dinfo[0]); void* scan = malloc(dinfo[1] ? dinfo[1] : 1);  // exact sizes again
        const long place[4] = {0, 0, 0, 0};
        int again[8];
        if (vtx_jpeg_describe(p, (long)d.size(), bits, again, desc, dinfo[0], scan, dinfo[1], place) == 0 && memcmp(again, dinfo, sizeof again) == 0) ++ok;
        else { fprintf(stderr, "second call disagrees with the first\n"); return 1; }
        free(desc); free(scan); free(p);
    }
    printf("described %ld refused %ld\n", ok, refused);
    return 0;
}
