// ehr_arrive.h -- how the composite stage's workgroups are counted in: the part's XCDs and the number of arrivals each
// XCD's counter ends at.  Plain C++ (no HIP header), so that a host program can check the
// arithmetic by brute force (tests/native/comp_arrivals_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define EHR_HD __host__ __device__
#else
#define EHR_HD
#endif

namespace ehr {

// The part's XCDs: workgroup w of a 1-D grid runs on XCD w % VB_XCDS (observed, used for L2 locality only)
constexpr int VB_XCDS = 8;
constexpr int VB_XCD_BITS = __builtin_ctz(VB_XCDS);
static_assert(VB_XCDS == 1 << VB_XCD_BITS, "a workgroup finds its XCD with a mask and a shift");
EHR_HD constexpr int vb_xcd_share(int n) { return (n + VB_XCDS - 1) >> VB_XCD_BITS; }  // ceil(n / XCDs)
EHR_HD constexpr int vb_xcd_round_up(int n) { return (n + VB_XCDS - 1) & ~(VB_XCDS - 1); }

// How many of XCD `xcd`'s `per` composite workgroups (block xcd + VB_XCDS k, k < per) have work in the call's last launch:
// an item of the XCD's contiguous run (wave slot 4 k + wave), a tile of the zero fill (nfill tiles, four per workgroup in
// block order) or link boxes to re-arm (nlbox ints, 256 per workgroup).  Each is a prefix in k, so their union is the
// longest one.  A function of the launch's tables only: every workgroup, and the finisher for every XCD, gets the same
// number.
EHR_HD constexpr int vb_comp_arrivals(int xcd, int per, int nitems, int nfill, int nlbox) {
    const int share = vb_xcd_share(nitems);
    const int left = nitems - xcd * share;
    const int mine = left < 0 ? 0 : (left < share ? left : share);  // items of this XCD
    int n = (mine + 3) >> 2;
    const int fwg = (nfill + 3) >> 2, lwg = (nlbox + 255) >> 8;  // workgroups (in block order) with a fill tile / boxes
    const int nf = fwg > xcd ? vb_xcd_share(fwg - xcd) : 0, nl = lwg > xcd ? vb_xcd_share(lwg - xcd) : 0;
    n = n > nf ? n : nf;
    n = n > nl ? n : nl;
    return n < per ? n : per;
}
// What the finisher (workgroup per - 1 of XCD 0, which never counts itself) waits for on XCD xcd's counter.  (Several
// counters per XCD were measured and left out: profiles/atomic_spread.md.)
EHR_HD constexpr int vb_comp_expected(int xcd, int per, int nitems, int nfill, int nlbox) {
    const int n = vb_comp_arrivals(xcd, per, nitems, nfill, nlbox);
    return n - ((xcd == 0 && per - 1 < n) ? 1 : 0);
}

}  // namespace ehr

#undef EHR_HD
