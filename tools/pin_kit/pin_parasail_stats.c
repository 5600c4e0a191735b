/*
 * pin_parasail_stats.c — SKETCH, not built by any Makefile: what a maintainer with libparasail 2.4.3 runs to pin the
 * stats-mode assumptions A.8-A.11 behind fadehip_sw_stats_batch, the way pin_parasail.c pins the
 * annotate ones.  Reads stats_pairs.tsv (query <TAB> reference per line) and prints
 * score end_query end_ref matches similar length per pair; compare with Context.sw_stats_batch on the same pairs.
 *   cc -O2 pin_parasail_stats.c -lparasail -o pin_parasail_stats && ./pin_parasail_stats < stats_pairs.tsv
 */
#include <parasail.h>
#include <stdio.h>
#include <string.h>

int main(void) {
    parasail_matrix_t *m = parasail_matrix_create("ACTGN", 10, -5);  /* stats.d:87 Parasail("ACTGN", 3, 8, 10, -5) */
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char *tab = strchr(line, '\t');
        if (!tab) continue;
        *tab = 0;
        char *r = tab + 1;
        r[strcspn(r, "\r\n")] = 0;
        /* dparasail's aligner!("sw","stats","striped","16") */
        parasail_result_t *res = parasail_sw_stats_striped_16(line, (int)strlen(line), r, (int)strlen(r), 3, 8, m);
        printf("%d\t%d\t%d\t%d\t%d\t%d\n", parasail_result_get_score(res), parasail_result_get_end_query(res),
               parasail_result_get_end_ref(res), parasail_result_get_matches(res), parasail_result_get_similar(res),
               parasail_result_get_length(res));
        parasail_result_free(res);
    }
    parasail_matrix_free(m);
    return 0;
}
