// Brute-force check of the composite stage's arrival arithmetic (easyhec_amd/csrc/ehr_arrive.h), a host program:
// for every launch shape below, the number of arrivals the finisher expects on an XCD's counter must equal the number of
// workgroups that really have work there, counted the way vb_composite_kernel hands work out.
// Prints "ok <cases>" and exits 0, or prints the first mismatches and exits 1.
#include <stdio.h>

#include "../../easyhec_amd/csrc/ehr_arrive.h"

using namespace ehr;

// does workgroup k of XCD xcd (block xcd + VB_XCDS k of `per` per XCD) have work?
static bool has_work(int xcd, int k, int nitems, int nfill, int nlbox) {
    const int blk = xcd + VB_XCDS * k;
    // items: the XCD's contiguous run, wave slot 4 k + wave takes item ibeg + slot
    const int share = (nitems + VB_XCDS - 1) / VB_XCDS;
    const int ibeg = xcd * share, iend = ibeg + share < nitems ? ibeg + share : nitems;
    for (int wave = 0; wave < 4; wave++)
        if (ibeg + 4 * k + wave < iend) return true;
    // zero fill: tile t = 4 blk + wave
    for (int wave = 0; wave < 4; wave++)
        if (4 * blk + wave < nfill) return true;
    // link boxes: int 256 blk + tid
    return 256 * blk < nlbox;
}

int main() {
    const int pers[] = {1, 2, 3, 24}, fills[] = {0, 1, 5, 33, 97, 800}, boxes[] = {0, 1, 256, 257, 1024, 8192};
    long cases = 0;
    int bad = 0;
    for (int per : pers)
        for (int nitems = 0; nitems <= 200; nitems++)
            for (int nfill : fills)
                for (int nlbox : boxes) {
                    for (int xcd = 0; xcd < VB_XCDS; xcd++) {
                        // the count is a prefix: workgroup k has work exactly when k < vb_comp_arrivals
                        const int n = vb_comp_arrivals(xcd, per, nitems, nfill, nlbox);
                        for (int k = 0; k < per; k++)
                            if (has_work(xcd, k, nitems, nfill, nlbox) != (k < n) && bad++ < 10)
                                printf("prefix: per %d nitems %d nfill %d nlbox %d xcd %d k %d n %d\n", per, nitems, nfill, nlbox, xcd, k, n);
                        int brute = 0;  // the finisher (workgroup per - 1 of XCD 0) never counts itself
                        for (int k = 0; k < per; k++)
                            brute += has_work(xcd, k, nitems, nfill, nlbox) && !(xcd == 0 && k == per - 1);
                        const int want = vb_comp_expected(xcd, per, nitems, nfill, nlbox);
                        if (want != brute && bad++ < 10)
                            printf("expected: per %d nitems %d nfill %d nlbox %d xcd %d: expected %d, counted %d\n", per, nitems, nfill, nlbox,
                                   xcd, want, brute);
                        cases++;
                    }
                }
    if (bad) {
        printf("FAILED: %d mismatches\n", bad);
        return 1;
    }
    printf("ok %ld\n", cases);
    return 0;
}
