// FaceSightings (include/frt/sightings.h) as a C++11 caller sees it.  The first part needs no GPU: creating a tracker and a book does no
// device work, and a refused creation throws.  With the argument "update" one face is followed for three frames on the device, its stream
// is closed, and the one sighting is drained: the sharpest of the three shots is the best one.
//   sightings_demo [update]
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "frt/sightings.h"

int main(int argc, char **) {
    FaceTracker trk(1, 4, 1, 8);
    bool refused = false;
    try {
        FaceSightings none(trk, 0);
    } catch (const std::logic_error &) {
        refused = true;
    }
    frt_sighting_options opt = {FRT_SHOT_RANK_SHARPNESS, 1, 1};
    FaceSightings book(trk, 16, &opt);
    if (!refused || !book.keepsCrops() || sizeof(frt_sighting) != 96) return 1;
    std::printf("book created\n");
    if (argc < 2) return 0;

    const size_t crop = (size_t)112 * 112 * 3;
    const float sharp[3] = {5.f, 9.f, 7.f};
    for (int i = 0; i < 3; ++i) {
        std::vector<frt_face_result> res(1, frt_face_result());
        res[0].box.x1 = 10, res[0].box.y1 = 10, res[0].box.x2 = 50, res[0].box.y2 = 50;
        res[0].box.score = 0.9f;
        res[0].match_idx = -1;
        res[0].valid = 1;
        std::vector<float> e(8, 0.f), tpl;
        e[i] = 1.f;
        std::vector<struct frt_face_quality> q(1);  // (value-initialised: all zero)
        q[0].present = 1;
        q[0].sharpness = sharp[i];
        const std::vector<uint8_t> crops(crop, (uint8_t)(i + 1));
        const std::vector<frt_track_result> tracks = trk.update(res, e, std::vector<int>(), nullptr, &tpl);
        book.update(res, tracks, e, tpl, q, crops);
    }
    book.close(0);
    int counters[4];
    const std::vector<Sighting> out = book.drain(4, counters);
    if (out.size() != 1) return 2;
    const frt_sighting &r = out[0].record;
    std::printf("sighting track %d ticks %d..%d reason %d hits %d shots %d best tick %d sharpness %g crop %d embed %g\n", r.track_id, r.first_tick,
                r.last_tick, r.reason, r.hits, r.n_shots, r.best_tick, r.best_sharpness, out[0].bestCrop[0], out[0].bestEmbed[1]);
    return r.reason == FRT_SIGHTING_CLOSED && r.hits == 3 && r.n_shots == 3 && r.best_tick == 1 && out[0].bestCrop[crop - 1] == 2 &&
                   out[0].bestEmbed[1] == 1.f && counters[0] == 1 && counters[3] == 1
               ? 0
               : 3;
}
