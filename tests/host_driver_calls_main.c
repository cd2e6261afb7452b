/* tests/host_driver_calls_main.c — TEST INFRASTRUCTURE: a caller that makes SEVERAL calls of the folder-level entry
 * points in one process, so that tests reach what the driver keeps between calls (the cached encoders and pinned
 * buffers) and what a failed call leaves for the next one.  Linked with csrc/encoder_host.c and
 * tests/host_driver_standin.c; the loader is the raw-pixel one of tests/raw_loader_main.c (int32 W, H, C, then W*H*C bytes).
 *
 *   host_driver_calls_main SCRIPT
 *
 * SCRIPT is a text file, one command per line, words separated by blanks (so no blanks in paths):
 *   call IMAGES BITS VIDEO QUALITY strict|full   mpeg_encode_procedure_region
 *   call IMAGES BITS VIDEO QUALITY env           mpeg_encode_procedure (the region comes from EC504_ENCODE_REGION)
 *   env NAME [VALUE]                             setenv, or unsetenv without a value
 *   threads N                                    encoder_set_host_threads
 *   release                                      encoder_release_cache
 *   noloader | loader                            unregister / register the image loader
 *   reset                                        the stand-in's call counters back to 0
 * Every line runs whatever the call before it returned.  After each call one line goes to stdout,
 *   == call <number> returned <rc> create=<n> alloc=<n> encode=<n>
 * with the stand-in's counters; the driver's own messages of that call stand in front of it.  Exit status 0 unless the
 * script cannot be read or holds a line that is none of the above (2). */
#include <string.h>
#define EC504_NO_STB
#include "encoder.h"

void standin_counts(int out[3]);
void standin_reset_counts(void);

static unsigned char *load_raw(char const *path, int *w, int *h, int *c, int desired) {
    (void)desired;
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    int hdr[3];
    unsigned char *px = NULL;
    if (fread(hdr, sizeof hdr, 1, f) == 1 && hdr[0] > 0 && hdr[1] > 0 && hdr[2] > 0) {
        size_t n = (size_t)hdr[0] * hdr[1] * hdr[2];
        px = (unsigned char *)malloc(n);
        if (px && fread(px, 1, n, f) != n) {
            free(px);
            px = NULL;
        }
        *w = hdr[0], *h = hdr[1], *c = hdr[2];
    }
    fclose(f);
    return px;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *script = fopen(argv[1], "r");
    if (!script) return 2;
    encoder_set_image_loader(load_raw, free);
    char line[2048];
    int calls = 0, bad = 0;
    while (fgets(line, sizeof line, script)) {
        char *w[7];
        int n = 0;
        for (char *t = strtok(line, " \t\r\n"); t && n < 7; t = strtok(NULL, " \t\r\n")) w[n++] = t;
        if (n == 0 || w[0][0] == '#') continue;
        if (strcmp(w[0], "call") == 0 && n == 6) {
            int rc, counts[3];
            if (strcmp(w[5], "env") == 0) rc = mpeg_encode_procedure(w[1], w[2], w[3], atoi(w[4]));
            else rc = mpeg_encode_procedure_region(w[1], w[2], w[3], atoi(w[4]), strcmp(w[5], "full") == 0);
            standin_counts(counts);
            printf("== call %d returned %d create=%d alloc=%d encode=%d\n", ++calls, rc, counts[0], counts[1], counts[2]);
            fflush(stdout);
        } else if (strcmp(w[0], "env") == 0 && n == 3) {
            setenv(w[1], w[2], 1);
        } else if (strcmp(w[0], "env") == 0 && n == 2) {
            unsetenv(w[1]);
        } else if (strcmp(w[0], "threads") == 0 && n == 2) {
            encoder_set_host_threads(atoi(w[1]));
        } else if (strcmp(w[0], "release") == 0 && n == 1) {
            encoder_release_cache();
        } else if (strcmp(w[0], "noloader") == 0 && n == 1) {
            encoder_set_image_loader(NULL, NULL);
        } else if (strcmp(w[0], "loader") == 0 && n == 1) {
            encoder_set_image_loader(load_raw, free);
        } else if (strcmp(w[0], "reset") == 0 && n == 1) {
            standin_reset_counts();
        } else {
            fprintf(stderr, "host_driver_calls_main: cannot read the line that starts with '%s'\n", w[0]);
            bad = 2;
        }
    }
    fclose(script);
    return bad;
}
