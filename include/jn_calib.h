/* jn_calib.h — C ABI of the calibration-file reader / writer of libjn_stereo.so.  Host only.
 *
 * The reference's `main` reads K1, K2, D1, D2, R, T, XR, XT from an OpenCV FileStorage YAML (point_cloud.cpp:530-540,
 * calibration/amrl_jackal_webcam_stereo.yml).  This is that subset, without OpenCV:
 *   %YAML:1.0                              first line (optional `---` after it)
 *   name: !!opencv-matrix                  a matrix: `rows`, `cols`, `dt` (d or f) and `data: [ ... ]`, the list possibly over several lines
 *   name: [ v, v, v ]                      a plain sequence (how the shipped file stores T); accepted for any entry with the right count
 * Shapes: K1, K2, R, XR 3x3; D1, D2 1x5 or 5x1; T, XT 3x1 or 1x3.  Unknown top-level keys are skipped; `#` starts a comment.
 * XR / XT may be absent: they come back as identity / zero, the README's starting point (see jn_ground.h for what to do next).
 * calib_width / calib_height are not in the file and are left as the caller set them.
 */
#ifndef JN_CALIB_H
#define JN_CALIB_H

#include <stdint.h>
#include "jn_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_CALIB_K1 1
#define JN_CALIB_K2 2
#define JN_CALIB_D1 4
#define JN_CALIB_D2 8
#define JN_CALIB_R 16
#define JN_CALIB_T 32
#define JN_CALIB_XR 64
#define JN_CALIB_XT 128
#define JN_CALIB_STEREO 63        /* K1 | K2 | D1 | D2 | R | T: what a file must hold */

/* `present` (may be NULL) receives the mask of the entries found.  JN_ERR_INVALID — and calib, XR, XT, present untouched — for a NULL
 * path / calib / XR / XT, a file that cannot be read, a missing %YAML header, a missing stereo entry, a wrong shape, a `dt` other than d / f,
 * a `data` list that is truncated, too long or holds something that is not a number, or an entry given twice.  Never exits. */
jn_status jn_calib_load_yaml(const char* path, jn_stereo_calib* calib, double XR[9], double XT[3], int32_t* present);

/* Writes all eight entries as !!opencv-matrix with %.17g, so that load(save(x)) == x bit for bit (finite values; the file format has no
 * spelling for NaN or infinity: JN_ERR_INVALID).  JN_ERR_INVALID also for a NULL argument or a path that cannot be written. */
jn_status jn_calib_save_yaml(const char* path, const jn_stereo_calib* calib, const double XR[9], const double XT[3]);

#ifdef __cplusplus
}
#endif
#endif /* JN_CALIB_H */
