// engine_file_check FILE — parses a flat engine file with the library's host-only parser and exits 0 when
// it is accepted, 2 (with the parser's message on stderr) when it is rejected, 1 on a usage error.  Host code only:
// `make -C dcfp_amd/csrc engine_file_check`, optionally with SANITIZE="-fsanitize=address,undefined
// -fno-sanitize-recover=all" - the program the corrupted-file tests run.
#include <stdio.h>
#include <string.h>

#include "engine_file.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 1;
    }
    dcfp_efile::File f;
    char err[256] = "";
    if (!dcfp_efile::load(argv[1], f, err, sizeof(err))) {
        fprintf(stderr, "rejected: %s\n", err);
        return 2;
    }
    size_t names = 0;
    for (const dcfp_efile::Record& r : f.records) names += strlen(f.name(r));   // (every name is a string in the file)
    printf("ok: format %d, %d records (%zu name bytes), %d buffers, %d tensors, %zu weight bytes, input table %s\n",
           f.meta.format, f.meta.n_records, names, f.meta.n_buffers, f.meta.n_tensors, f.weights_size,
           f.has_input ? "yes" : "no");
    return 0;
}
