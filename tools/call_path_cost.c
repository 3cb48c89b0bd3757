/* Wall time per call of the host path of a process call that launches nothing: an empty batch (batch = 0) runs every
 * argument check of the entry point and returns before any device work.  Several builds of the library in one process,
 * one handle each, rounds interleaved and rotated (as tools/ab_libs.py does for the launch path); name the same library
 * twice for its own run-to-run spread.
 *   build:  gcc -O2 -o tools/call_path_cost tools/call_path_cost.c -ldl
 *   usage:  tools/call_path_cost libA.so libB.so ...        (paths as given; needs a GPU: sa_create)
 * Prints, per library and entry point, the median, minimum and maximum over the rounds of ns per call. */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

enum { ROUNDS = 31, CALLS = 2000000, MAXLIBS = 8 };

typedef int (*create_fn)(int, void **);
typedef int (*destroy_fn)(void *);
typedef int (*q15_out_fn)(void *, const void *, void *, int, int, void *);
typedef int (*spectra_fn)(void *, const void *, void *, int, int, int, void *);

struct lib {
    const char *path;
    void *h;
    destroy_fn destroy;
    q15_out_fn q15_out;
    spectra_fn spectra;
    double ns[2][ROUNDS];
};

static double now_ns(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e9 * (double)t.tv_sec + (double)t.tv_nsec;
}

static int cmp(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

int main(int argc, char **argv)
{
    static struct lib libs[MAXLIBS];
    const int n = argc - 1;
    if (n < 1 || n > MAXLIBS) {
        fprintf(stderr, "usage: %s libA.so [libB.so ...]\n", argv[0]);
        return 2;
    }
    for (int i = 0; i < n; ++i) {
        struct lib *l = &libs[i];
        l->path = argv[i + 1];
        void *so = dlopen(l->path, RTLD_NOW | RTLD_LOCAL);
        if (!so) {
            fprintf(stderr, "%s\n", dlerror());
            return 1;
        }
        create_fn create = (create_fn)dlsym(so, "sa_create");
        l->destroy = (destroy_fn)dlsym(so, "sa_destroy");
        l->q15_out = (q15_out_fn)dlsym(so, "sa_process_q15_out");
        l->spectra = (spectra_fn)dlsym(so, "sa_spectra_q15");
        if (!create || !l->destroy || !l->q15_out || !l->spectra || create(0, &l->h) != 0) {
            fprintf(stderr, "%s: no handle\n", l->path);
            return 1;
        }
    }
    /* addresses that are never read: an empty batch returns before the pointers are looked at */
    const void *in = (const void *)(size_t)4096;
    void *out = (void *)(size_t)8192;
    int bad = 0;
    for (int r = -1; r < ROUNDS; ++r)                       /* round -1: warm-up, not recorded */
        for (int k = 0; k < n; ++k) {
            struct lib *l = &libs[(k + (r + 1)) % n];
            for (int f = 0; f < 2; ++f) {
                const double t0 = now_ns();
                if (f == 0)
                    for (int c = 0; c < CALLS; ++c) bad |= l->q15_out(l->h, in, out, 0, c & 1 ? 0x2009C : 0, NULL);
                else
                    for (int c = 0; c < CALLS; ++c) bad |= l->spectra(l->h, in, out, 0, 2, c & 1 ? 4096 : 0, NULL);
                if (r >= 0) l->ns[f][r] = (now_ns() - t0) / CALLS;
            }
        }
    if (bad) {
        fprintf(stderr, "an empty-batch call was refused\n");
        return 1;
    }
    printf("%d rounds of %d empty-batch calls, ns per call\n", (int)ROUNDS, (int)CALLS);
    for (int f = 0; f < 2; ++f)
        for (int i = 0; i < n; ++i) {
            double *v = libs[i].ns[f];
            qsort(v, ROUNDS, sizeof *v, cmp);
            printf("%-20s %-40s #%d  median %7.2f  min %7.2f  max %7.2f\n", f ? "sa_spectra_q15" : "sa_process_q15_out",
                   libs[i].path, i, v[ROUNDS / 2], v[0], v[ROUNDS - 1]);
        }
    for (int i = 0; i < n; ++i) libs[i].destroy(libs[i].h);
    return 0;
}
