// FaceTracker's motion methods (include/frt/tracker.h) as a C++11 caller sees them: the setting round-trips, a refused set throws and
// changes nothing, and reading the velocities while motion is off throws.  That part needs no GPU (creating a tracker and switching motion
// on does no device work); with the argument "update" it also runs one coasting return on the device.
//   track_motion_demo [update]
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "frt/tracker.h"

static frt_face_result face(int x) {
    frt_face_result r = frt_face_result();
    r.box.x1 = x, r.box.y1 = 0, r.box.x2 = x + 47, r.box.y2 = 47;
    r.box.score = 0.9f;
    r.match_idx = -1;
    r.valid = 1;
    return r;
}

int main(int argc, char **) {
    FaceTracker trk(1, 2, 1, 8);
    if (trk.getMotion() != 0) return 1;
    trk.setMotion(256);
    trk.setMotion(64);
    int refused = 0;
    for (int bad = -1; bad <= 257; bad += 258) {
        try {
            trk.setMotion(bad);
        } catch (const std::logic_error &) {
            ++refused;
        }
    }
    if (refused != 2 || trk.getMotion() != 64) return 2;
    trk.setMotion(0);
    try {
        trk.motion(0);
    } catch (const std::logic_error &) {
        ++refused;
    }
    if (refused != 3) return 3;
    trk.setMotion(256);
    std::printf("motion %d\n", trk.getMotion());
    if (argc < 2) return 0;

    // a face that moves 8 pixels per update is seen three times, hidden for four updates, and comes back 40 pixels on: the same track,
    // by the overlap with the predicted box
    std::vector<float> e(8, 0.f);
    std::vector<frt_track_assoc> assoc;
    std::vector<frt_face_result> unseen(1, frt_face_result());
    unseen[0].match_idx = -1;
    int first = -1;
    for (int i = 0; i < 3; ++i) first = trk.update(std::vector<frt_face_result>(1, face(8 * i)), e)[0].track_id;
    for (int i = 0; i < 4; ++i) trk.update(unseen, e);
    std::vector<frt_bbox> pred;
    std::vector<int32_t> vel = trk.motion(0, &pred);
    std::vector<frt_track_result> back = trk.update(std::vector<frt_face_result>(1, face(56)), e, assoc);
    std::printf("track %d %d how %d gap %d ovr %g vel %d %d pred %d %d\n", first, back[0].track_id, assoc[0].how, assoc[0].gap, assoc[0].ovr, vel[0], vel[1],
                pred[0].x1, pred[0].x2);
    return first == 0 && back[0].track_id == 0 && assoc[0].how == FRT_TRACK_ASSOC_IOU && assoc[0].gap == 4 && assoc[0].ovr == 1.f ? 0 : 4;
}
