// Pipeline::find_entities_along_segments and Pipeline::first_hits of the C++ host mirror (include/render_engine_hip.hpp): what lies along a line, on a
// handful of instances: before the first frame (the query uploads the world), with the shooter excluded, with a filter, after an instance was added
// between frames, with a segment that ends exactly on a face, and a refused segment.
#include <algorithm>
#include <cstdio>
#include <limits>
#include <tuple>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

using Rec = std::tuple<uint32_t, uint32_t, float, float>;
static std::vector<Rec> sorted(const std::vector<re_segment_hit> &hits) {
    std::vector<Rec> out;
    for (const re_segment_hit &h : hits) out.emplace_back(h.query, h.entity_id, h.t_enter, h.t_exit);
    std::sort(out.begin(), out.end());
    return out;
}

int main() {
    Camera camera = CameraBuilder({ 1280, 720 }).with_position(vec3(1000.0f, 1000.0f, 1150.0f)).with_direction(vec3(0.0f, 0.0f, -1.0f)).with_far_draw_distance(1000.0f).build();
    Pipeline pipeline(16384, 64);
    const StaticAABB box{ { -1.0f, 1.0f }, { -1.0f, 1.0f }, { -1.0f, 1.0f } };
    std::vector<EntityId> made;
    auto place = [&](float x, float z, bool is_static) {
        pipeline.register_model_instances(ModelId{ 2, 0 }, 1, box, [&](Pipeline &p, const std::vector<EntityId> &created, StaticAABB aabb) {
            EntityTransformationBuilder b(created[0], is_static, std::nullopt, false);
            b.with_translation(Position::new_(vec3(x, 1000.0f, z)));
            b.apply_choices(aabb, p);
            made.push_back(created[0]);
        });
    };
    place(970.0f, 1000.0f, false); place(1023.0f, 1000.0f, false); place(1025.0f, 1000.0f, true);      // x in [969, 971], [1022, 1024] (on the section border), [1024, 1026]
    const EntityId a = made[0], b = made[1], c = made[2];
    // segment 0: the shot of a along x, from its centre over 64 units: a itself (from inside: t_enter 0), b and c; segment 1: the same with a excluded;
    // segment 2: from x = 1020 to the face x = 1022 of b: a touch at t = 1; segment 3: nobody
    using S = Pipeline::Segment;
    const std::vector<S> segs{ S{ vec3(970.0f, 1000.0f, 1000.0f), vec3(1034.0f, 1000.0f, 1000.0f) }, S{ vec3(970.0f, 1000.0f, 1000.0f), vec3(1034.0f, 1000.0f, 1000.0f), a },
                               S{ vec3(1020.0f, 1000.0f, 1000.0f), vec3(1022.0f, 1000.0f, 1000.0f) }, S{ vec3(970.0f, 500.0f, 1000.0f), vec3(1034.0f, 500.0f, 1000.0f) } };
    const Rec a0{ 0u, a, 0.0f, 1.0f / 64.0f }, b0{ 0u, b, 52.0f / 64.0f, 54.0f / 64.0f }, c0{ 0u, c, 54.0f / 64.0f, 56.0f / 64.0f };
    const Rec b1{ 1u, b, 52.0f / 64.0f, 54.0f / 64.0f }, c1{ 1u, c, 54.0f / 64.0f, 56.0f / 64.0f }, b2{ 2u, b, 1.0f, 1.0f };
    std::vector<Rec> want{ a0, b0, c0, b1, c1, b2 };
    std::sort(want.begin(), want.end());
    const std::vector<re_segment_hit> hits = pipeline.find_entities_along_segments(segs);
    if (sorted(hits) != want) return fail("records before the first frame");
    const auto first = Pipeline::first_hits(hits, segs.size());
    if (!(first[0] && first[0]->entity_id == a && first[1] && first[1]->entity_id == b && first[1]->t_enter == 52.0f / 64.0f && first[2] && first[2]->entity_id == b && !first[3]))
        return fail("first hits");
    if (sorted(pipeline.find_entities_along_segments(segs, 0u, RE_F_STATIC)) != std::vector<Rec>{ a0, b0, b1, b2 }) return fail("forbid RE_F_STATIC");
    if (sorted(pipeline.find_entities_along_segments(segs, RE_F_STATIC)) != std::vector<Rec>{ c0, c1 }) return fail("need RE_F_STATIC");
    pipeline.execute(camera, 1.0f / 60.0f);
    place(1002.0f, 1000.0f, false);                                    // registered after frames have run: appended; x in [1001, 1003]
    const EntityId late = made[3];
    std::vector<Rec> want2 = want; want2.push_back(Rec{ 0u, late, 31.0f / 64.0f, 33.0f / 64.0f }); want2.push_back(Rec{ 1u, late, 31.0f / 64.0f, 33.0f / 64.0f });
    std::sort(want2.begin(), want2.end());
    const std::vector<re_segment_hit> hits2 = pipeline.find_entities_along_segments(segs);
    if (sorted(hits2) != want2) return fail("records with an instance added later");
    if (Pipeline::first_hits(hits2, segs.size())[1]->entity_id != late) return fail("the later instance is the first hit of the shot");
    if (!pipeline.find_entities_along_segments({}).empty()) return fail("no segments, no records");
    try { pipeline.find_entities_along_segments({ S{ vec3(0.0f, 0.0f, 0.0f), vec3(std::numeric_limits<float>::infinity(), 0.0f, 0.0f) } }); return fail("a non-finite segment is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a non-finite segment is RE_E_ARG"); }
    std::printf("OK segment queries through the C++ mirror\n");
    return 0;
}
