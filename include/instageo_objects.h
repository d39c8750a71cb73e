/* instageo_objects.h -- C ABI of the object-level comparison of class maps (objects.hip), a companion of instageo_hip.h in the same shared
 * library: same conventions (int return: IG_OK = 0 or a negative IG_ERR_* with the text in ig_last_error(); device pointers unless a
 * parameter is called a HOST array; the trailing `stream` is a hipStream_t).  instageo_amd._lib binds the prototypes below beside those
 * of instageo_hip.h, and the torch custom ops are generated from them in the same way. */
#ifndef INSTAGEO_OBJECTS_H
#define INSTAGEO_OBJECTS_H
#ifdef __cplusplus
extern "C" {
#endif
/* First 28 bits of the MD5 of this header as the library was built against it (the Makefile passes it): the loader refuses a library
 * built against another revision, as ig_header_stamp does for instageo_hip.h. */
int ig_objects_header_stamp(void);
/* Object-level comparison of two labelled class maps (objects.hip; not in the reference).  gt, pred (n, HW) int8 class maps with their
 * ig_ccl_label labels gt_labels, pred_labels (n, HW) int32 (a component's smallest pixel index, -1 at fill) and ig_region_area areas
 * gt_area, pred_area (n, HW) int32 (the pixel count at root positions): a label is the address of its region's class and area.
 * n * HW <= 2^31 - 1 per call.  Integer work on integers: every result is bit-identical from run to run and independent of `capacity`;
 * no kernel waits on another thread or workgroup.  n = 0 returns IG_OK without touching a pointer.
 * ig_object_pairs: the sparse overlap table.  A pixel q of image i counts iff gt_labels[q] >= 0 and pred_labels[q] >= 0, under the key
 *   ((uint64)(i * HW + gt_labels[q]) << 32) | (uint32)pred_labels[q].  keys uint64[capacity], counts uint32[capacity]: an open-addressed
 *   table in caller-owned memory, capacity a power of two in [1024, 2^30], the empty key is all ones; BOTH arrays are cleared by the
 *   entry point before the tally (nothing an earlier launch left there is read).  Slot = a fixed 64-bit mix of the key (the murmur3
 *   finaliser), linear probing: a 64-bit compare-and-swap on keys, then an integer add on counts; lanes of a wave that hold the same key
 *   insert once, with their number.  A lane that has probed `capacity` slots sets bit 0 of *status (device int, OR-ed, never cleared
 *   here) and drops its count: the table is then not valid.  With status 0 the SET of (key, count) entries is unique: count = the
 *   pixels two regions share; slot positions are not unique and mean nothing.
 * ig_object_match: one thread per slot.  A non-empty slot (i, g, p, cnt) has cg = gt[i HW + g], cp = pred[i HW + p], ag = gt_area[i HW + g],
 *   ap = pred_area[i HW + p], u = ag + ap - cnt; it is skipped unless cg == cp, 0 <= cg < ncls (2 <= ncls <= 127), ag >= min_area and
 *   ap >= min_area (min_area >= 1).  num, den = HOST arrays of K thresholds num[k] / den[k], 1 <= K <= 10, den[k] >= 1 and
 *   1/2 <= num[k] / den[k] < 1.  The pair is a match at k iff cnt * den[k] > num[k] * u in 64-bit integers: IoU STRICTLY above the
 *   threshold, so that from 1/2 up a region matches at most one region of the other map and the matching is unique.  Accumulated (the
 *   caller zeroes) into DEVICE uint64 tables: tp[K][ncls] += 1, iou_q[K][ncls] += (cnt * 2^25 + u) / (2 u) = the IoU in units of 2^-24
 *   rounded half up.  Integer sums: they do not depend on any order and add across calls and ranks.  The 2 * K * ncls cells are
 *   aggregated per workgroup in LDS (at most 20 KiB: always) and reach memory as one 64-bit add per non-empty cell and workgroup.
 * ig_object_count: n_regions[ncls] (DEVICE uint64, accumulated) += the root positions (labels[q] == q - i * HW) with 0 <= cls[q] < ncls
 *   and area[q] >= min_area: the regions of one map, called once for gt and once for pred.  LDS histogram, one add per non-empty cell
 *   and workgroup. */
int ig_object_pairs(const int* gt_labels, const int* pred_labels, unsigned long long* keys, unsigned* counts, long capacity, int* status,
                    int n, long HW, void* stream);
int ig_object_match(const unsigned long long* keys, const unsigned* counts, long capacity, const signed char* gt, const signed char* pred,
                    const int* gt_area, const int* pred_area, const int* num, const int* den, int K, unsigned long long* tp,
                    unsigned long long* iou_q, int n, long HW, int ncls, int min_area, void* stream);
int ig_object_count(const signed char* cls, const int* labels, const int* area, unsigned long long* n_regions, int n, long HW, int ncls,
                    int min_area, void* stream);
#ifdef __cplusplus
}
#endif
#endif
