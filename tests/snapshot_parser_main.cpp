// Stand-alone driver of the snapshot parser for a host sanitizer build (tests/test_snapshot_format_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a subprocess).  Includes nothing of the project but snapshot_format.h.
//   argv[1] = a file holding one valid blob.
// Every truncation length 0 .. size - 1 and every single-byte corruption (two bit patterns per byte) is parsed from a heap buffer of EXACTLY the
// length handed to the parser, so a read past `nbytes` is a heap-buffer-overflow report.  Exit status 0 and one "OK ..." line when the valid blob
// is accepted and nothing else is.
#include "../streamvoiceanon_amd/csrc/snapshot/snapshot_format.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static int parse_exact(const std::vector<uint8_t>& bytes, size_t n) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
    if (n) memcpy(buf.get(), bytes.data(), n);
    sva::snap::Header h;
    return sva::snap::parse(n ? buf.get() : buf.get(), (long)n, true, &h);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s blob\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("fopen"); return 2; }
    std::vector<uint8_t> blob;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) blob.insert(blob.end(), tmp, tmp + got);
    fclose(f);
    if (parse_exact(blob, blob.size()) != sva::snap::kOk) { fprintf(stderr, "the valid blob was refused\n"); return 1; }
    long n_trunc = 0, n_corrupt = 0;
    for (size_t n = 0; n < blob.size(); ++n, ++n_trunc)
        if (parse_exact(blob, n) == sva::snap::kOk) { fprintf(stderr, "accepted a blob truncated to %zu bytes\n", n); return 1; }
    for (size_t i = 0; i < blob.size(); ++i)
        for (uint8_t flip : {(uint8_t)0x01, (uint8_t)0x80}) {
            std::vector<uint8_t> bad(blob);
            bad[i] ^= flip;
            ++n_corrupt;
            if (parse_exact(bad, bad.size()) == sva::snap::kOk) { fprintf(stderr, "accepted a blob with byte %zu corrupted\n", i); return 1; }
        }
    {   // a trailing byte is not a valid blob either
        std::vector<uint8_t> longer(blob);
        longer.push_back(0);
        if (parse_exact(longer, longer.size()) == sva::snap::kOk) { fprintf(stderr, "accepted a blob with a trailing byte\n"); return 1; }
    }
    printf("OK %ld truncations %ld corruptions refused\n", n_trunc, n_corrupt);
    return 0;
}
