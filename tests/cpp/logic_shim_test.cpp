// The entity-logic surface of the C++ host mirror (include/render_engine_hip.hpp): write_entity_type / remove_entity_type / register_entity_logic and
// execute(.., logic = true), on a handful of entities around the camera.  Types written before the first frame travel with the upload, types of instances
// registered after frames have run with re_add_entities, and a type written or removed later goes straight to the library.
#include <algorithm>
#include <cstdio>
#include <tuple>
#include <vector>

#include "render_engine_hip.hpp"

using namespace render_engine;

static int fail(const char *what) { std::printf("FAIL: %s\n", what); return 1; }

using Rec = std::tuple<uint32_t, unsigned, unsigned, unsigned>;
static std::vector<Rec> sorted(const std::vector<re_logic_call> &calls) {
    std::vector<Rec> out;
    for (const re_logic_call &c : calls) out.emplace_back(c.entity_id, c.logic_index, c.which, c.times);
    std::sort(out.begin(), out.end());
    return out;
}

int main() {
    constexpr uint64_t USER = 0x1001, ROCK = 0x1002, MINE = 0x1003;
    Camera camera = CameraBuilder({ 1280, 720 }).with_position(vec3(1000.0f, 1000.0f, 1150.0f)).with_direction(vec3(0.0f, 0.0f, -1.0f)).with_far_draw_distance(1000.0f).build();
    Pipeline pipeline(16384, 64);
    const StaticAABB box{ { -1.0f, 1.0f }, { -1.0f, 1.0f }, { -1.0f, 1.0f } };
    const EntityId user = pipeline.register_user_entity(vec3(1000.0f, 1000.0f, 1150.0f), StaticAABB{ { -5.0f, 5.0f }, { -5.0f, 5.0f }, { -5.0f, 5.0f } }, ModelId{ 6, 0 });
    std::vector<EntityId> made;
    auto place = [&](float x, float z, bool is_static) {
        pipeline.register_model_instances(ModelId{ 2, 0 }, 1, box, [&](Pipeline &p, const std::vector<EntityId> &created, StaticAABB aabb) {
            EntityTransformationBuilder b(created[0], is_static, std::nullopt, false);
            b.with_translation(Position::new_(vec3(x, 1000.0f, z)));
            b.apply_choices(aabb, p);
            made.push_back(created[0]);
        });
    };
    place(970.0f, 1000.0f, false); place(980.0f, 1000.0f, false); place(990.0f, 1000.0f, true);      // where the sample scene has its wormhole and mine producer: in the frustum, outside the logic culler
    const EntityId rock = made[0], mine = made[1], fixed = made[2];
    pipeline.write_entity_type(user, USER); pipeline.write_entity_type(rock, ROCK); pipeline.write_entity_type(mine, MINE); pipeline.write_entity_type(fixed, MINE);
    const uint16_t i_user = pipeline.register_entity_logic(USER, RE_LOGIC_ENTITY), i_mine = pipeline.register_entity_logic(MINE, RE_LOGIC_ENTITY);
    if (pipeline.register_entity_logic(MINE, RE_LOGIC_RANDOM) != i_mine) return fail("a second function of a type keeps the type's index");
    if (i_user != 0 || i_mine != 1) return fail("logic indices follow the registration order");

    FrameResult plain = pipeline.execute(camera, 1.0f / 60.0f);
    if (!plain.logic_calls.empty()) return fail("execute without logic fills no call list");
    // the user entity and the mine (entity + random logic); the rock's type carries no logic, the static instance is not processed
    const std::vector<Rec> want{ Rec{ user, i_user, RE_LOGIC_ENTITY, 1u }, Rec{ mine, i_mine, RE_LOGIC_ENTITY | RE_LOGIC_RANDOM, 1u } };
    FrameResult fr = pipeline.execute(camera, 1.0f / 60.0f, false, false, false, /*logic=*/true);
    if (sorted(fr.logic_calls) != want) return fail("call list of the uploaded world");

    place(985.0f, 1005.0f, false);                                    // registered after frames have run: appended, typed with its registration
    const EntityId late = made[3];
    pipeline.write_entity_type(late, MINE);
    fr = pipeline.execute(camera, 1.0f / 60.0f, false, false, true, true);
    std::vector<Rec> want2 = want; want2.push_back(Rec{ late, i_mine, RE_LOGIC_ENTITY | RE_LOGIC_RANDOM, 1u }); std::sort(want2.begin(), want2.end());
    if (sorted(fr.logic_calls) != want2) return fail("call list with an instance added later");
    if (!pipeline.has_component(late, RE_ECS_BIT_TYPE_IDENTIFIER) || pipeline.has_component(rock, RE_ECS_BIT_TYPE_IDENTIFIER) != true) return fail("TypeIdentifier bit");

    pipeline.remove_entity_type(mine); pipeline.write_entity_type(rock, MINE);
    fr = pipeline.execute(camera, 1.0f / 60.0f, false, false, false, true);
    std::vector<Rec> want3{ Rec{ user, i_user, RE_LOGIC_ENTITY, 1u }, Rec{ rock, i_mine, RE_LOGIC_ENTITY | RE_LOGIC_RANDOM, 1u }, Rec{ late, i_mine, RE_LOGIC_ENTITY | RE_LOGIC_RANDOM, 1u } };
    std::sort(want3.begin(), want3.end());
    if (sorted(fr.logic_calls) != want3) return fail("call list after remove_entity_type / write_entity_type");
    if (pipeline.has_component(mine, RE_ECS_BIT_TYPE_IDENTIFIER)) return fail("TypeIdentifier bit after remove_entity_type");
    std::printf("OK logic calls through the C++ mirror\n");
    return 0;
}
