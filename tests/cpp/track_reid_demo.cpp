// FaceTracker's appearance methods (include/frt/tracker.h) as a C++11 caller sees them: the settings round-trip, a refused set throws and
// changes nothing, and the update overload that returns the association records is well-formed.  The first part needs no GPU (creating a
// tracker and setting it up does no device work); with the argument "update" it also runs one re-attach on the device.
//   track_reid_demo [update]
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "frt/tracker.h"

static frt_face_result face(int x1, int y1, int x2, int y2) {
    frt_face_result r = frt_face_result();
    r.box.x1 = x1, r.box.y1 = y1, r.box.x2 = x2, r.box.y2 = y2;
    r.box.score = 0.9f;
    r.match_idx = -1;
    r.valid = 1;
    return r;
}

int main(int argc, char **) {
    FaceTracker trk(1, 4, 1, 8);
    float reid = 0.f, minSim = 0.f;
    trk.getAppearance(reid, minSim);
    if (reid != FRT_TRACK_REID_OFF || minSim != FRT_TRACK_MIN_SIM_OFF) return 1;
    trk.setAppearance(0.5f, 0.25f);
    bool refused = false;
    try {
        trk.setAppearance(1.5f, 0.25f);
    } catch (const std::logic_error &) {
        refused = true;
    }
    trk.getAppearance(reid, minSim);
    if (!refused || reid != 0.5f || minSim != 0.25f) return 2;
    std::printf("appearance %g %g\n", reid, minSim);
    if (argc < 2) return 0;

    // one face, seen, unseen, and back at a box that does not overlap the first: the same track, by appearance
    std::vector<float> e(8, 0.f);
    e[3] = 1.f;
    std::vector<frt_track_assoc> assoc;
    std::vector<frt_face_result> seen(1, face(10, 10, 50, 50)), unseen(1, frt_face_result()), back(1, face(100, 100, 140, 140));
    unseen[0].match_idx = -1;
    std::vector<frt_track_result> t0 = trk.update(seen, e, assoc);
    trk.update(unseen, e);
    std::vector<frt_track_result> t2 = trk.update(back, e, assoc);
    std::printf("track %d %d how %d gap %d sim %g\n", t0[0].track_id, t2[0].track_id, assoc[0].how, assoc[0].gap, assoc[0].sim);
    return t0[0].track_id == 0 && t2[0].track_id == 0 && assoc[0].how == FRT_TRACK_ASSOC_APPEARANCE && assoc[0].gap == 1 && assoc[0].sim == 1.f ? 0 : 3;
}
