// Pipeline::find_entities_around and Pipeline::find_entities_within_reach of the C++ host mirror (include/render_engine_hip.hpp): who is within reach of an
// entity, on a handful of instances: before the first frame (the query uploads the world), keeping the asker, with a filter, after an instance was added
// between frames, an ask beyond the cap among answered ones, and refused batches.
#include <algorithm>
#include <cstdio>
#include <tuple>
#include <utility>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

using Pair = std::pair<uint32_t, uint32_t>;
static std::vector<Pair> sorted(const std::vector<re_box_hit> &hits) {
    std::vector<Pair> out;
    for (const re_box_hit &h : hits) out.emplace_back(h.query, h.entity_id);
    std::sort(out.begin(), out.end());
    return out;
}
using Rec = std::tuple<uint32_t, uint32_t, float, uint32_t>;
static std::vector<Rec> sorted(const std::vector<re_sphere_hit> &hits) {
    std::vector<Rec> out;
    for (const re_sphere_hit &h : hits) out.emplace_back(h.query, h.entity_id, h.dist_sq, h.side);
    std::sort(out.begin(), out.end());
    return out;
}
template <class T> static std::vector<T> sorted(std::vector<T> v) { std::sort(v.begin(), v.end()); return v; }

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
    using A = Pipeline::Around;
    // ask 0: a grown by 51 reaches to x = 1022, the minimum face of b: a touch; ask 1: the same, keeping itself; ask 2: b as it is touches c at x = 1024;
    // ask 3: c as it is touches b, whose maximum lies on the section border 1024: it sits in the lower section only
    const std::vector<A> asks{ A{ a, 51.0f }, A{ a, 51.0f, true }, A{ b, 0.0f }, A{ c, 0.0f } };
    const std::vector<Pair> want{ { 0u, b }, { 1u, a }, { 1u, b }, { 2u, c }, { 3u, b } };
    const auto got = pipeline.find_entities_around(asks);
    if (sorted(got.hits) != sorted(want)) return fail("box records before the first frame");
    if (got.status != std::vector<uint8_t>(4, RE_AROUND_OK)) return fail("status before the first frame");
    if (sorted(pipeline.find_entities_around(asks, 0u, RE_F_STATIC).hits) != sorted(std::vector<Pair>{ { 0u, b }, { 1u, a }, { 1u, b }, { 3u, b } })) return fail("forbid RE_F_STATIC");
    if (sorted(pipeline.find_entities_around(asks, RE_F_STATIC).hits) != sorted(std::vector<Pair>{ { 2u, c } })) return fail("need RE_F_STATIC");
    // the spheres around the Positions (the middles of the boxes): from x = 970 with reach 52, b begins 52 away (a touch, beyond its minimum x face), c 54;
    // keeping itself, a is inside its own box; c's Position is 1 beyond the maximum x face of b
    const std::vector<A> reach{ A{ a, 52.0f }, A{ a, 52.0f, true }, A{ c, 1.0f } };
    const std::vector<Rec> wants{ Rec{ 0u, b, 2704.0f, 1u }, Rec{ 1u, a, 0.0f, 0u }, Rec{ 1u, b, 2704.0f, 1u }, Rec{ 2u, b, 1.0f, 16u } };
    const auto gots = pipeline.find_entities_within_reach(reach);
    if (sorted(gots.hits) != sorted(wants)) return fail("sphere records before the first frame");
    pipeline.execute(camera, 1.0f / 60.0f);
    place(1002.0f, 1000.0f, false);                                    // registered after frames have run: appended; x in [1001, 1003]: 30 from a's box
    const EntityId late = made[3];
    std::vector<Pair> want2 = want; want2.push_back({ 0u, late }); want2.push_back({ 1u, late });
    if (sorted(pipeline.find_entities_around(asks).hits) != sorted(want2)) return fail("box records with an instance added later");
    const auto late_asks = pipeline.find_entities_around({ A{ late, 19.0f }, A{ late, 18.0f } });      // the late instance asks: b is 19 away
    if (sorted(late_asks.hits) != std::vector<Pair>{ { 0u, b } }) return fail("the instance added later asks");
    // an ask beyond the cap (40 atomic lengths of reach) is refused alone
    const auto mixed = pipeline.find_entities_around({ A{ b, 0.0f }, A{ a, 2560.0f }, A{ c, 0.0f } });
    if (mixed.status != std::vector<uint8_t>{ RE_AROUND_OK, RE_AROUND_TOO_LARGE, RE_AROUND_OK }) return fail("status of an ask beyond the cap");
    if (sorted(mixed.hits) != std::vector<Pair>{ { 0u, c }, { 2u, b } }) return fail("the neighbours of a refused ask are answered");
    if (!pipeline.find_entities_around({}).hits.empty() || !pipeline.find_entities_within_reach({}).hits.empty()) return fail("no asks, no records");
    try { pipeline.find_entities_around({ A{ a, 1.0f }, A{ 4242u, 1.0f } }); return fail("an unknown entity is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("an unknown entity is RE_E_ARG"); }
    try { pipeline.find_entities_within_reach({ A{ a, -1.0f } }); return fail("a negative reach is refused"); }
    catch (const Error &e) { if (e.code != RE_E_ARG) return fail("a negative reach is RE_E_ARG"); }
    if (sorted(pipeline.find_entities_around(asks).hits) != sorted(want2)) return fail("records after refused calls");
    std::printf("OK queries asked by entity through the C++ mirror\n");
    return 0;
}
