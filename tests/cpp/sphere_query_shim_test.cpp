// Pipeline::find_entities_within_radius and Pipeline::nearest_hits of the C++ host mirror (include/render_engine_hip.hpp): who is within r of a point, on a
// handful of instances: before the first frame (the query uploads the world), with the asking entity excluded, with a filter, after an instance was added
// between frames, with spheres that only touch a face and an edge, and refused spheres.
#include <algorithm>
#include <cstdio>
#include <limits>
#include <tuple>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

using Rec = std::tuple<uint32_t, uint32_t, float, uint32_t>;
static std::vector<Rec> sorted(const std::vector<re_sphere_hit> &hits) {
    std::vector<Rec> out;
    for (const re_sphere_hit &h : hits) out.emplace_back(h.query, h.entity_id, h.dist_sq, h.side);
    std::sort(out.begin(), out.end());
    return out;
}
static std::vector<Rec> sorted(std::vector<Rec> recs) { std::sort(recs.begin(), recs.end()); return recs; }

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
    // sphere 0: around the centre of a, radius 52: a itself (from inside: 0, side 0) and b, whose face x = 1022 it touches (52 * 52, side 1); c is 54 away;
    // sphere 1: radius 54 with a excluded: b, and c by a touch; sphere 2: a 3-4-5 touch over the edge x = 1026, y = 1001 of c (beyond both maxima: side 16 | 32);
    // sphere 3: nobody
    using S = Pipeline::Sphere;
    const std::vector<S> sph{ S{ vec3(970.0f, 1000.0f, 1000.0f), 52.0f }, S{ vec3(970.0f, 1000.0f, 1000.0f), 54.0f, a }, S{ vec3(1030.0f, 1004.0f, 1000.0f), 5.0f },
                              S{ vec3(970.0f, 500.0f, 1000.0f), 10.0f } };
    const Rec a0{ 0u, a, 0.0f, 0u }, b0{ 0u, b, 2704.0f, 1u }, b1{ 1u, b, 2704.0f, 1u }, c1{ 1u, c, 2916.0f, 1u }, c2{ 2u, c, 25.0f, 48u };
    const std::vector<Rec> want = sorted(std::vector<Rec>{ a0, b0, b1, c1, c2 });
    const std::vector<re_sphere_hit> hits = pipeline.find_entities_within_radius(sph);
    if (sorted(hits) != want) return fail("records before the first frame");
    const auto nearest = Pipeline::nearest_hits(hits, sph.size());
    if (!(nearest[0] && nearest[0]->entity_id == a && nearest[0]->dist_sq == 0.0f && nearest[1] && nearest[1]->entity_id == b && nearest[1]->dist_sq == 2704.0f && nearest[2] &&
          nearest[2]->entity_id == c && !nearest[3]))
        return fail("nearest hits");
    if (sorted(pipeline.find_entities_within_radius(sph, 0u, RE_F_STATIC)) != sorted(std::vector<Rec>{ a0, b0, b1 })) return fail("forbid RE_F_STATIC");
    if (sorted(pipeline.find_entities_within_radius(sph, RE_F_STATIC)) != sorted(std::vector<Rec>{ c1, c2 })) return fail("need RE_F_STATIC");
    pipeline.execute(camera, 1.0f / 60.0f);
    place(1002.0f, 1000.0f, false);                                    // registered after frames have run: appended; x in [1001, 1003]: 31 from the centre of a
    const EntityId late = made[3];
    std::vector<Rec> want2 = want; want2.push_back(Rec{ 0u, late, 961.0f, 1u }); want2.push_back(Rec{ 1u, late, 961.0f, 1u });
    const std::vector<re_sphere_hit> hits2 = pipeline.find_entities_within_radius(sph);
    if (sorted(hits2) != sorted(want2)) return fail("records with an instance added later");
    if (Pipeline::nearest_hits(hits2, sph.size())[1]->entity_id != late) return fail("the later instance is the nearest of the excluding sphere");
    if (!pipeline.find_entities_within_radius({}).empty()) return fail("no spheres, no records");
    try { pipeline.find_entities_within_radius({ S{ vec3(std::numeric_limits<float>::infinity(), 0.0f, 0.0f), 1.0f } }); return fail("a non-finite sphere is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a non-finite sphere is RE_E_ARG"); }
    try { pipeline.find_entities_within_radius({ S{ vec3(1000.0f, 1000.0f, 1000.0f), -1.0f } }); return fail("a negative radius is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a negative radius is RE_E_ARG"); }
    if (sorted(pipeline.find_entities_within_radius(sph)) != sorted(want2)) return fail("records after refused calls");
    std::printf("OK sphere queries through the C++ mirror\n");
    return 0;
}
