// Pipeline::find_first_along_segments and Pipeline::find_nearest_within_radius of the C++ host mirror (include/render_engine_hip.hpp): what each segment hits
// first and who is nearest to each point, reduced on the device, on a handful of instances: before the first frame (the query uploads the world), with the
// asking entity excluded, with a filter, after an instance was added between frames, a tie that the lower id wins, a query without a hit -- each answer
// against the hand-worked one and against first_hits / nearest_hits of the full answer of the same pipeline, field by field.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

template <class Hit> static bool same(const std::vector<std::optional<Hit>> &a, const std::vector<std::optional<Hit>> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].has_value() != b[i].has_value()) return false;
        if (a[i] && std::memcmp(&*a[i], &*b[i], sizeof(Hit)) != 0) return false;      // bit for bit in all four fields
    }
    return true;
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
    using S = Pipeline::Sphere;
    using G = Pipeline::Segment;
    // sphere 0: around the centre of a, radius 60: a itself from inside (0, side 0); sphere 1: the same with a excluded: b, 52 away (2704, side 1), before c;
    // sphere 2: on the face x = 1024 that b and c share, radius 3: both at 0 from inside, the lower id wins; sphere 3: nobody
    const std::vector<S> sph{ S{ vec3(970.0f, 1000.0f, 1000.0f), 60.0f }, S{ vec3(970.0f, 1000.0f, 1000.0f), 60.0f, a }, S{ vec3(1024.0f, 1000.0f, 1000.0f), 3.0f },
                              S{ vec3(970.0f, 500.0f, 1000.0f), 10.0f } };
    // segment 0: along x from 960 to 1040 through a, b and c: a first, entered at 9 / 80; segment 1: the same with a excluded: b at 62 / 80;
    // segment 2: down y onto the face x = 1024 that b and c share: both entered at 9 / 10, the lower id wins; segment 3: nobody
    const std::vector<G> seg{ G{ vec3(960.0f, 1000.0f, 1000.0f), vec3(1040.0f, 1000.0f, 1000.0f) }, G{ vec3(960.0f, 1000.0f, 1000.0f), vec3(1040.0f, 1000.0f, 1000.0f), a },
                              G{ vec3(1024.0f, 1010.0f, 1000.0f), vec3(1024.0f, 1000.0f, 1000.0f) }, G{ vec3(960.0f, 500.0f, 1000.0f), vec3(1040.0f, 500.0f, 1000.0f) } };
    const EntityId low = b < c ? b : c;

    auto nearest = pipeline.find_nearest_within_radius(sph);                     // before the first frame
    if (!(nearest.size() == 4 && nearest[0] && nearest[0]->query == 0u && nearest[0]->entity_id == a && nearest[0]->dist_sq == 0.0f && nearest[0]->side == 0u)) return fail("nearest of sphere 0");
    if (!(nearest[1] && nearest[1]->query == 1u && nearest[1]->entity_id == b && nearest[1]->dist_sq == 2704.0f && nearest[1]->side == 1u)) return fail("nearest with the asking entity excluded");
    if (!(nearest[2] && nearest[2]->entity_id == low && nearest[2]->dist_sq == 0.0f && nearest[2]->side == 0u)) return fail("a tie of spheres falls to the lower id");
    if (nearest[3]) return fail("a sphere without a hit");
    if (!same(nearest, Pipeline::nearest_hits(pipeline.find_entities_within_radius(sph), sph.size()))) return fail("nearest against nearest_hits");

    auto first = pipeline.find_first_along_segments(seg);
    if (!(first.size() == 4 && first[0] && first[0]->query == 0u && first[0]->entity_id == a && first[0]->t_enter == 9.0f / 80.0f && first[0]->t_exit == 11.0f / 80.0f)) return fail("first of segment 0");
    if (!(first[1] && first[1]->query == 1u && first[1]->entity_id == b && first[1]->t_enter == 62.0f / 80.0f && first[1]->t_exit == 64.0f / 80.0f)) return fail("first with the asking entity excluded");
    if (!(first[2] && first[2]->entity_id == low && first[2]->t_enter == 9.0f / 10.0f && first[2]->t_exit == 1.0f)) return fail("a tie of segments falls to the lower id");
    if (first[3]) return fail("a segment without a hit");
    if (!same(first, Pipeline::first_hits(pipeline.find_entities_along_segments(seg), seg.size()))) return fail("first against first_hits");

    // the filter: without the static c, and the static c alone
    auto dyn = pipeline.find_nearest_within_radius(sph, 0u, RE_F_STATIC);
    if (!(dyn[2] && dyn[2]->entity_id == b) || !same(dyn, Pipeline::nearest_hits(pipeline.find_entities_within_radius(sph, 0u, RE_F_STATIC), sph.size()))) return fail("nearest, forbid RE_F_STATIC");
    auto stat = pipeline.find_first_along_segments(seg, RE_F_STATIC);
    if (!(stat[0] && stat[0]->entity_id == c && stat[0]->t_enter == 64.0f / 80.0f && stat[2] && stat[2]->entity_id == c) ||
        !same(stat, Pipeline::first_hits(pipeline.find_entities_along_segments(seg, RE_F_STATIC), seg.size()))) return fail("first, need RE_F_STATIC");

    pipeline.execute(camera, 1.0f / 60.0f);
    place(1002.0f, 1000.0f, false);                                    // registered after frames have run: x in [1001, 1003], between a and b
    const EntityId late = made[3];
    nearest = pipeline.find_nearest_within_radius(sph);
    if (!(nearest[1] && nearest[1]->entity_id == late && nearest[1]->dist_sq == 961.0f)) return fail("the later instance is the nearest of the excluding sphere");
    if (!same(nearest, Pipeline::nearest_hits(pipeline.find_entities_within_radius(sph), sph.size()))) return fail("nearest against nearest_hits, later");
    first = pipeline.find_first_along_segments(seg);
    if (!(first[1] && first[1]->entity_id == late && first[1]->t_enter == 41.0f / 80.0f)) return fail("the later instance is the first of the excluding segment");
    if (!same(first, Pipeline::first_hits(pipeline.find_entities_along_segments(seg), seg.size()))) return fail("first against first_hits, later");

    if (!pipeline.find_nearest_within_radius({}).empty() || !pipeline.find_first_along_segments({}).empty()) return fail("no queries, no records");
    try { pipeline.find_nearest_within_radius({ S{ vec3(1000.0f, 1000.0f, 1000.0f), -1.0f } }); return fail("a negative radius is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a negative radius is RE_E_ARG"); }
    try { pipeline.find_first_along_segments({ G{ vec3(std::numeric_limits<float>::infinity(), 0.0f, 0.0f), vec3(0.0f, 0.0f, 0.0f) } }); return fail("a non-finite segment is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a non-finite segment is RE_E_ARG"); }
    if (!same(pipeline.find_first_along_segments(seg), first) || !same(pipeline.find_nearest_within_radius(sph), nearest)) return fail("answers after refused calls");
    std::printf("OK first hits and nearest entities through the C++ mirror\n");
    return 0;
}
